// vit_demap_dev.h -- what the two demappers share, vit_ofdm.hip (from the FFT) and vit_ofdm_td.hip (from the samples):
// the per-carrier soft-decision rule, the place of a data symbol's soft bytes, and the launch bookkeeping, templated on
// the kernels' argument structs (OfdmArgs, TdArgs) over their same-named fields.  A TU that includes it turns
// contraction off.
#pragma once
#include <cfloat>

#include "vit_csi_dev.h"
#include "vit_internal.h"

namespace vit_demap {

typedef uint32_t u32;
typedef uint64_t u64;

// the two soft bytes of one carrier (low byte: bit n, next byte: bit n + K) from a = z[l], b = z[l-1]
__device__ __forceinline__ u32 soft_pair(float ar, float ai, float br, float bi, float gain) {
    const float re = ar * br + ai * bi;
    const float im = ai * br - ar * bi;
    const float nrm = __builtin_fabsf(re) + __builtin_fabsf(im);
    u32 q = 0x8080u;
    if (nrm >= 0x1p-64f && nrm <= FLT_MAX) q = vit_csi::csi_pair(re, im, gain / nrm);  // false for NaN
    return q;
}

// where the 2K soft bytes of data symbol s of frame t go: d_fic, or a CIF row of the ring
template <typename Args>
__device__ __forceinline__ uint8_t* soft_dst(const Args& A, u64 t, u32 s) {
    const u32 nb = 2u * A.K;
    if (s < A.fic_syms) return A.fic + (t * A.fic_syms + s) * nb;
    const u32 m = s - A.fic_syms, c = m / A.per;
    u64 row = A.first_row + t * A.cifs + c;
    if (row >= A.nrows) row -= A.nrows;
    return A.ring + row * A.row_bytes + A.col + (u64)(m - c * A.per) * nb;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
constexpr u32 RUN_MAX = 25;  // symbols per workgroup at most: the one extra row or transform per run is then <= 4 %

// The demapping fields of the arguments: the shape, the data symbols [lo, hi) that have a destination, the destinations.
template <typename Args>
void set_outputs(Args& A, const vit_ofdm_shape& shape, float gain, uint8_t* d_fic, const vit_cif_ring* ring, u64 col) {
    A.K = shape.ncarriers;
    A.fic_syms = shape.fic_syms;
    A.cifs = shape.cifs;
    A.per = (shape.nsyms - 1u - shape.fic_syms) / shape.cifs;
    A.lo = d_fic ? 0u : shape.fic_syms;
    A.hi = ring ? shape.nsyms - 1u : shape.fic_syms;
    A.gain = gain;
    A.fic = d_fic;
    if (ring) {
        A.ring = const_cast<uint8_t*>(ring->d_base);  // this call is the ring's writer
        A.row_bytes = ring->row_bytes;
        A.nrows = ring->nrows;
        A.first_row = ring->first_row;
        A.col = col;
    }
}

// Splits the symbols [lo, hi) of every frame into runs, one workgroup each: about 8 workgroups per CU over the whole
// grid (all the CU can hold: 4 waves each), RUN_MAX symbols at most.  Returns the grid, 0 if there is nothing to do.
template <typename Args>
u64 split_runs(Args& A, int64_t nframes) {
    if (nframes <= 0 || A.hi <= A.lo) return 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const u64 target = 8ull * (u64)vit_device_cus(dev);
    const u32 nsym = A.hi - A.lo;
    u64 rpf = (target + (u64)nframes - 1) / (u64)nframes;
    if (rpf > nsym) rpf = nsym;
    u32 run = (u32)((nsym + rpf - 1) / rpf);
    if (run > RUN_MAX) run = RUN_MAX;
    A.run = run;
    A.runs = (nsym + run - 1) / run;
    return (u64)nframes * A.runs;
}

}  // namespace vit_demap
