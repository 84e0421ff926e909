// vit_ti.hip -- MSC time de-interleaving on the device (EN 300 401 clause 12): a standalone de-interleave, and one fused
// into the depuncturing expansion of vit_punct.hip.
//
// Byte i of logical frame n of a call lies in ring row (first_row + n + F[i mod 16]) mod nrows, column col + i, with
// F[k] = k bit-reversed (include/viterbi_amd.h, vit_cif_ring).  Gathered byte by byte from global memory, one output
// dword would touch up to 4 rows, a wavefront about 16 rows x 2 lines per load, and the 16 frames that share a row's
// lines would run in workgroups on different XCDs.  Instead one workgroup owns a window of columns and a run of
// consecutive frames.  It keeps 32 consecutive rows of its window in LDS (row r in slot r mod 32): frames n ... n+15
// need rows n ... n+30, so each iteration adds the 16 rows that are new - 16-byte loads, clamped to the window, so no
// byte outside the call's columns is read, issued one iteration ahead into registers - and produces 16 frames from LDS.
// Every row of the call is read once per window, plus 15 rows at the start of each run.
//   standalone: windows of at most 1024 columns; a lane writes 16 consecutive bytes of one frame (one unaligned
//               16-byte store; a window's last chunk is clamped to end at the window's end and rewrites a few bytes).
//   fused:      windows of at most 200 trellis steps (<= 800 transmitted bytes, the profile being uniform); a lane
//               expands one step as vit_depunct_kernel does - the step table, v_perm_b32 against the erasure word, one
//               coalesced output dword - with its <= 4 transmitted bytes read from LDS.
#include "vit_internal.h"
#include "vit_punct_dev.h"

namespace {

typedef uint32_t u32;
typedef uint64_t u64;
constexpr u32 TPB = 256;
constexpr u32 SLOTS = 32;        // LDS row slots: 16 frames need 31 rows
constexpr u32 FRAMES_PER_IT = 16;
constexpr u32 MAX_WCOLS = 1024;  // standalone: columns per window
// fused: trellis steps per window (<= 4 bytes each).  200 keeps a window's LDS under 26 KiB, so 6 workgroups fit per CU;
// at 256, DAB+ frames need 32 KiB windows and 4 fit: the DAB+ chain runs at 1.11x instead of 1.02x of the chain on
// de-interleaved input, and the FIC's 194-step windows are the same (profiles/r07_ti_window_ab.json)
constexpr u32 MAX_WSTEPS = 200;

struct Ring {
    const uint8_t* base;
    u64 row_bytes;
    u64 nrows;
    u64 first_row;
};

// F[k]: k with its 4 bits reversed
__device__ __forceinline__ u32 frev(u32 i) { return __builtin_bitreverse32(i) >> 28; }

// One iteration's new rows (at most 16) of a window of L <= 1024 bytes, in 16-byte chunks spread over the workgroup:
// at most CHUNKS_PER_LANE per lane.  load_rows fetches them into registers - the next iteration's rows are loaded
// before the current one's expansion, so their latency hides behind it (a barrier waits for LDS operations only) -
// and store_rows writes them to their LDS slots (row r at rows + (r % 32) * wb, wb a multiple of 16).  Every load lies
// inside the columns [lo, lo + L): a row's last chunk is clamped to end at lo + L and stores only the bytes the previous
// chunk did not; a window shorter than 16 bytes takes byte loads.
constexpr u32 CHUNKS_PER_LANE = FRAMES_PER_IT * (MAX_WCOLS / 16u) / TPB;
struct Staged {
    uint4 v[CHUNKS_PER_LANE];
};

__device__ __forceinline__ void load_rows(const Ring& ring, u64 lo, u32 L, u64 r0, u64 r1, Staged& st) {
    const u32 nch = (L + 15u) / 16u, total = (u32)(r1 - r0) * nch;
#pragma unroll
    for (u32 c = 0; c < CHUNKS_PER_LANE; c++) {
        const u32 e = threadIdx.x + c * TPB;
        if (e >= total) break;
        const u32 rr = e / nch, k = e - rr * nch;
        u64 row = ring.first_row + r0 + rr;
        if (row >= ring.nrows) row -= ring.nrows;
        const uint8_t* src = ring.base + row * ring.row_bytes + lo;
        if (L >= 16u) {
            const u32 a = 16u * k < L - 16u ? 16u * k : L - 16u;
            __builtin_memcpy(&st.v[c], src + a, 16);  // unaligned global_load_dwordx4
        } else {
            u32 w[4] = {0, 0, 0, 0};
#pragma unroll
            for (u32 j = 0; j < 16; j++)
                if (j < L) w[j >> 2] |= (u32)src[j] << (8u * (j & 3u));
            st.v[c] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
}

__device__ __forceinline__ void store_rows(u32 L, u64 r0, u64 r1, const Staged& st, uint8_t* rows, u32 wb) {
    const u32 nch = (L + 15u) / 16u, total = (u32)(r1 - r0) * nch;
#pragma unroll
    for (u32 c = 0; c < CHUNKS_PER_LANE; c++) {
        const u32 e = threadIdx.x + c * TPB;
        if (e >= total) break;
        const u32 rr = e / nch, k = e - rr * nch;
        uint8_t* dst = rows + (u32)((r0 + rr) % SLOTS) * wb;
        const u32 want = 16u * k, a = L < 16u ? 0u : (want < L - 16u ? want : L - 16u);
        if (a == want && L >= 16u) {
            *reinterpret_cast<uint4*>(dst + a) = st.v[c];
        } else {
            const u32 skip = want - a, w[4] = {st.v[c].x, st.v[c].y, st.v[c].z, st.v[c].w};
#pragma unroll
            for (u32 j = 0; j < 16; j++)
                if (j >= skip && j < L) dst[a + j] = (uint8_t)(w[j >> 2] >> (8u * (j & 3u)));
        }
    }
}

// Rows of the first iteration: the first 15 into LDS, the next up to 16 into registers.
__device__ __forceinline__ void prologue(const Ring& ring, u64 lo, u32 L, u64 begin, u64 rend, Staged& st, uint8_t* rows,
                                         u32 wb) {
    load_rows(ring, lo, L, begin, begin + 15u, st);
    store_rows(L, begin, begin + 15u, st, rows, wb);
    load_rows(ring, lo, L, begin + 15u, rend, st);
}

// Window w of blockIdx.x % nwin, run of frames [c * fpw, min(nframes, (c + 1) * fpw)) with c = blockIdx.x / nwin.
struct Run {
    u64 begin, end;
};
__device__ __forceinline__ Run run_of(u32 nwin, u64 nframes, u32 fpw) {
    const u64 c = blockIdx.x / nwin;
    Run r;
    r.begin = c * fpw;
    r.end = r.begin + fpw < nframes ? r.begin + fpw : nframes;
    return r;
}
// end of the rows frames nb ... nb+15 of the run need (only the call's nframes + 15 rows are ever read)
__device__ __forceinline__ u64 rows_end(u64 nb, const Run& run) { return nb + 31u < run.end + 15u ? nb + 31u : run.end + 15u; }

// Standalone: frame n's ncols bytes to out + n*ncols.  LDS: SLOTS * wcols bytes.
__global__ __launch_bounds__(TPB) void vit_ti_kernel(Ring ring, u64 col, u32 ncols, u32 wcols, u32 nwin, u64 nframes,
                                                     u32 fpw, uint8_t* __restrict__ out) {
    extern __shared__ uint4 lds_ti[];
    uint8_t* rows = reinterpret_cast<uint8_t*>(lds_ti);
    const u32 c0 = (blockIdx.x % nwin) * wcols, c1 = c0 + wcols < ncols ? c0 + wcols : ncols, L = c1 - c0;
    const Run run = run_of(nwin, nframes, fpw);
    Staged st;
    prologue(ring, col + c0, L, run.begin, rows_end(run.begin, run), st, rows, wcols);
    const u32 nch = (L + 15u) / 16u;
    for (u64 nb = run.begin; nb < run.end; nb += FRAMES_PER_IT) {
        store_rows(L, nb + 15u, rows_end(nb, run), st, rows, wcols);
        if (nb + FRAMES_PER_IT < run.end) load_rows(ring, col + c0, L, nb + 31u, rows_end(nb + FRAMES_PER_IT, run), st);
        __syncthreads();
        const u32 nf = run.end - nb < FRAMES_PER_IT ? (u32)(run.end - nb) : FRAMES_PER_IT;
        for (u32 e = threadIdx.x; e < nf * nch; e += TPB) {
            const u32 fl = e / nch, k = e - fl * nch;
            const u32 slot0 = (u32)(nb + fl);  // the frame's F = 0 row (mod 32)
            uint8_t* dst = out + (nb + fl) * ncols + c0;
            if (L >= 16u) {
                const u32 a = 16u * k < L - 16u ? 16u * k : L - 16u, i = c0 + a;
                u32 w[4] = {0, 0, 0, 0};
#pragma unroll
                for (u32 j = 0; j < 16; j++) {
                    const u32 slot = (slot0 + frev(i + j)) % SLOTS;
                    w[j >> 2] |= (u32)rows[slot * wcols + a + j] << (8u * (j & 3u));
                }
                const uint4 v = make_uint4(w[0], w[1], w[2], w[3]);
                __builtin_memcpy(dst + a, &v, 16);  // unaligned global_store_dwordx4
            } else {
                for (u32 j = 0; j < L; j++) dst[j] = rows[((slot0 + frev(c0 + j)) % SLOTS) * wcols + j];
            }
        }
        __syncthreads();
    }
}

// Fused: frame n's expanded symbols (T dwords) to out + n*T, from transmitted bytes at columns [col, col + P).
// Window w covers steps [w*S, min(T, (w+1)*S)); its transmitted bytes are [b0, b1).  LDS: SLOTS * wb bytes, then the
// window's step table (S entries: byte offset within the window | keep nibble << 16).
__global__ __launch_bounds__(TPB) void vit_ti_depunct_kernel(Ring ring, u64 col, SegTab tab, u32 T, u32 S, u32 nwin, u32 wb,
                                                             u64 nframes, u32 fpw, u32 erasure4, u32* __restrict__ out) {
    extern __shared__ uint4 lds_ti[];
    uint8_t* rows = reinterpret_cast<uint8_t*>(lds_ti);
    u32* stab = reinterpret_cast<u32*>(rows + SLOTS * wb);
    __shared__ u32 seltab[16];
    const u32 s0 = (blockIdx.x % nwin) * S, s1 = s0 + S < T ? s0 + S : T, Sw = s1 - s0;
    u32 b0, b1, nib;
    locate(s0, tab, b0, nib);
    locate(s1, tab, b1, nib);  // (s1 == T gives P)
    for (u32 t = threadIdx.x; t < Sw; t += TPB) {
        u32 off;
        locate(s0 + t, tab, off, nib);
        stab[t] = (off - b0) | nib << 16;
    }
    if (threadIdx.x < 16) seltab[threadIdx.x] = expand_sel(threadIdx.x);
    const Run run = run_of(nwin, nframes, fpw);
    const u32 L = b1 - b0;
    Staged st;
    prologue(ring, col + b0, L, run.begin, rows_end(run.begin, run), st, rows, wb);
    // lane -> (frame, step) of the flattened 16-frame x Sw-step block, advanced by TPB without a division
    const u32 dq = TPB / Sw, dr = TPB - dq * Sw;
    for (u64 nb = run.begin; nb < run.end; nb += FRAMES_PER_IT) {
        store_rows(L, nb + 15u, rows_end(nb, run), st, rows, wb);
        if (nb + FRAMES_PER_IT < run.end) load_rows(ring, col + b0, L, nb + 31u, rows_end(nb + FRAMES_PER_IT, run), st);
        __syncthreads();
        const u32 nf = run.end - nb < FRAMES_PER_IT ? (u32)(run.end - nb) : FRAMES_PER_IT;
        u32 fl = threadIdx.x / Sw, t = threadIdx.x - fl * Sw;
        while (fl < nf) {
            const u32 ent = stab[t], off = ent & 0xFFFFu, nb4 = ent >> 16, cnt = __builtin_popcount(nb4);
            const u32 slot0 = (u32)(nb + fl), i = b0 + off;
            u32 w = 0;
#pragma unroll
            for (u32 j = 0; j < 4; j++)
                if (j < cnt) w |= (u32)rows[((slot0 + frev(i + j)) % SLOTS) * wb + off + j] << (8u * j);
            out[(nb + fl) * T + s0 + t] = __builtin_amdgcn_perm(erasure4, w, seltab[nb4]);
            t += dr;
            fl += dq;
            if (t >= Sw) {
                t -= Sw;
                fl++;
            }
        }
        __syncthreads();
    }
}

// Frames per workgroup: about 4 workgroups per CU over the whole grid, at least one iteration's 16.
u32 frames_per_wg(int64_t nframes, u32 nwin) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const u64 target = 4ull * (u64)vit_device_cus(dev);
    u64 f = ((u64)nframes * nwin + target - 1) / target;
    f = (f + FRAMES_PER_IT - 1) / FRAMES_PER_IT * FRAMES_PER_IT;
    return (u32)(f < FRAMES_PER_IT ? FRAMES_PER_IT : f);
}

Ring ring_of(const vit_cif_ring& r) { return Ring{r.d_base, r.row_bytes, r.nrows, r.first_row}; }

}  // namespace

hipError_t vit_launch_time_deinterleave(const vit_cif_ring& ring, uint64_t col, uint32_t ncols, uint8_t* d_out,
                                        int64_t nframes, hipStream_t stream) {
    if (nframes <= 0 || ncols == 0) return hipSuccess;
    const u32 n0 = (ncols + MAX_WCOLS - 1) / MAX_WCOLS;
    const u32 wcols = ((ncols + n0 - 1) / n0 + 15u) / 16u * 16u, nwin = (ncols + wcols - 1) / wcols;  // none empty
    const u32 fpw = frames_per_wg(nframes, nwin);
    const u64 grid = ((u64)nframes + fpw - 1) / fpw * nwin;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vit_ti_kernel, dim3((unsigned)grid), dim3(TPB), (size_t)SLOTS * wcols, stream, ring_of(ring), (u64)col,
                       ncols, wcols, nwin, (u64)nframes, fpw, d_out);
    return hipGetLastError();
}

hipError_t vit_launch_depunct_ti(const vit_cif_ring& ring, uint64_t col, uint8_t* d_sym8, uint32_t framebits, int64_t nframes,
                                 const vit_punct_profile* profile, uint8_t erasure, hipStream_t stream) {
    SegTab tab = {};
    const int64_t P = vit_punct_length_host(profile, framebits, tab.start, tab.base);
    if (P < 0) return hipErrorInvalidValue;
    if (nframes <= 0) return hipSuccess;
    tab.nsegs = profile->nsegs;
    for (uint32_t k = 0; k < tab.nsegs; k++) tab.keep[k] = profile->seg[k].keep;
    const uint32_t T = framebits + VIT_TAIL;
    const u32 n0 = (T + MAX_WSTEPS - 1) / MAX_WSTEPS, S = (T + n0 - 1) / n0, nwin = (T + S - 1) / S;
    // a window's bytes: at most 4 per step, rounded up to the 16-byte slot stride
    const u32 wb = (4u * S + 15u) / 16u * 16u;
    const u32 fpw = frames_per_wg(nframes, nwin);
    const u64 grid = ((u64)nframes + fpw - 1) / fpw * nwin;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vit_ti_depunct_kernel, dim3((unsigned)grid), dim3(TPB), (size_t)SLOTS * wb + (size_t)S * sizeof(u32),
                       stream, ring_of(ring), (u64)col, tab, T, S, nwin, wb, (u64)nframes, fpw, 0x01010101u * erasure,
                       reinterpret_cast<u32*>(d_sym8));
    return hipGetLastError();
}
