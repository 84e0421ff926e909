// vit_host.h -- the host side shared by the units of the C ABI: vit_api.hip (process state, the per-thread context, the
// reference exports), vit_ring.hip (the ingest stage), vit_api_decode.hip (kernel choice and the entry points around the
// decoder) and vit_api_ofdm.hip (the receiver front).  The kernels' launchers are in vit_internal.h.
#pragma once
#include <emmintrin.h>

#include "vit_internal.h"

#define set_err vit_set_err
// `if (a rule is broken) return bad_arg(...)`: sets the error text like set_err and returns VIT_ERR_ARG
int bad_arg(const char* fmt, ...);

#define HIPCHK(call)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            set_err("%s failed: %s", #call, hipGetErrorString(e_));                        \
            return VIT_ERR_HIP;                                                            \
        }                                                                                  \
    } while (0)
// A launch (or another asynchronous call) that failed: fmt, with one %s for HIP's text, is what the caller sees.
inline bool launch_ok(const char* fmt, hipError_t e) {
    if (e != hipSuccess) set_err(fmt, hipGetErrorString(e));
    return e == hipSuccess;
}
#define LAUNCHCHK(fmt, call)                                                               \
    do {                                                                                   \
        if (!launch_ok(fmt, (call))) return VIT_ERR_HIP;                                   \
    } while (0)

// ---- vit_api.hip: process state and the calling thread's context -----------------------------------------------------
// VIT_OK, or VIT_ERR_NO_DEVICE with the probe's text as the error text
int hip_device_ready();
// the device of the host-buffer entry points (*_dev calls use the caller's current device); -1: none
int vit_default_device();
// what an exported entry point reads ONCE per call
struct DecodeMode {
    int kernel;
    bool ge;
};
DecodeMode decode_mode();
// this thread's own stream on device `dev`, which must be the current device; nullptr (error text set) on failure
hipStream_t vit_thread_stream(int dev);

// This thread's scratch on the caller's CURRENT device (the device its pointers and `stream` belong to, not the
// library's default device): the only way an entry point obtains it.  The buffers are shared by every call of the
// thread, whatever they keep in them; their reuse across the caller's streams is ordered by one event, which begin()
// makes `stream` wait on and end() records - after the last launch that touches the scratch.  A failed launch in between
// returns without end(): nothing is recorded.  Growth: 64 KiB at least, need + 25 %, hipFree before hipMalloc (which
// may synchronise the device).
class ScratchLease {
public:
    // sym_bytes of symbol scratch and desc_bytes of descriptor scratch, either may be 0
    int begin(size_t sym_bytes, size_t desc_bytes, hipStream_t stream);
    int end();
    template <class T> T* sym() const { return static_cast<T*>(sym_); }  // expanded or narrowed symbols, or a call's floats
    vit_frame_desc* desc() const { return static_cast<vit_frame_desc*>(desc_); }

private:
    void *sym_ = nullptr, *desc_ = nullptr;
    hipEvent_t ev_ = nullptr;
    hipStream_t stream_ = nullptr;
};

inline bool valid_framebits(uint32_t fb) { return fb <= VIT_MAX_FRAMEBITS && (fb & 1u) == 0; }

// u32 -> u8 (low byte) while copying a caller's symbols into pinned memory; n is a multiple of 8
inline void narrow_symbols(const unsigned int* src, uint8_t* dst, size_t n) {
    size_t i = 0;
    const __m128i lo = _mm_set1_epi32(0xFF);
    for (; i + 16 <= n; i += 16) {
        const __m128i a = _mm_and_si128(_mm_loadu_si128(reinterpret_cast<const __m128i*>(src + i)), lo);
        const __m128i b = _mm_and_si128(_mm_loadu_si128(reinterpret_cast<const __m128i*>(src + i + 4)), lo);
        const __m128i c = _mm_and_si128(_mm_loadu_si128(reinterpret_cast<const __m128i*>(src + i + 8)), lo);
        const __m128i d = _mm_and_si128(_mm_loadu_si128(reinterpret_cast<const __m128i*>(src + i + 12)), lo);
        // values are 0..255: the signed/unsigned saturating packs are exact
        _mm_storeu_si128(reinterpret_cast<__m128i*>(dst + i), _mm_packus_epi16(_mm_packs_epi32(a, b), _mm_packs_epi32(c, d)));
    }
    for (; i < n; i++) dst[i] = (uint8_t)src[i];
}

// ---- vit_api_decode.hip: kernel choice and dispatch ----------------------------------------------------------------------
// the analogue of setupdll.cpp:195-270's dispatcher: choose the kernel for a batch.  `choice` is the value of
// vit_set_kernel() READ ONCE by the exported entry point (a concurrent vit_set_kernel must not flip the decision
// between the check that sizes the scratch buffers and the launch).
enum { K_AUTO = 0, K_WAVE = 1, K_PACKED = 2, K_LATENCY = 3, K_PACKED8 = 4 };
// The 8-frames-per-wavefront kernel (vit_pk8.hip; round 3: 12 % fewer instructions per frame, 19 % slower than vit_pk.hip -
// two wavefronts per SIMD cannot hide the LDS round trips, profiles/r03_ab_pk8.txt) is an experiment: it is compiled in
// only with -DVIT_WITH_PK8 (viterbi.dll_amd/build.py: build(extra=["-DVIT_WITH_PK8"])).  The product library does not
// carry it: vit_set_kernel(4) then selects 0 (auto).
#ifdef VIT_WITH_PK8
constexpr int K_MAX = K_PACKED8;
#else
constexpr int K_MAX = K_LATENCY;
#endif
// which kernel runs a batch: the explicit choice, or for K_AUTO the latency kernel for launches that cannot fill
// the chip (<= VIT_LAT_MAX_FRAMES wavefronts) and the packed kernel otherwise; -1: the packed kernel was asked for and
// does not support max_framebits
int pick_kernel(int choice, uint32_t max_framebits, int64_t nframes);
// The one decode dispatch: picks the kernel once and launches it.  sym32: `symbols` are still in the reference ABI's u32
// format (deconvolve.cpp:158-165).  The packed and the latency kernel read them in place if they are 16-byte aligned
// (narrowing fused into their symbol loads); otherwise they are narrowed into the thread's scratch first.
int launch_decode(DecodeMode mode, const void* symbols, bool sym32, uint8_t* d_out, const vit_frame_desc* d_desc,
                  uint32_t framebits, uint32_t max_framebits, int64_t nframes, hipStream_t s);
// The rules of a CIF ring (include/viterbi_amd.h, vit_cif_ring) that every call shares, false (error text set) if one is
// broken: d_base (and the ring, if it may be NULL; null_fmt is the caller's wording) and first_row, then - behind the
// caller's own row-count rule - the columns [col, col + ncols).
bool ring_check_base(const char* who, const vit_cif_ring* ring, const char* null_fmt);
bool ring_check_cols(const char* who, const vit_cif_ring* ring, uint64_t col, uint64_t ncols);

// ---- vit_ring.hip: the ingest stage for concurrent deconvolve() callers ----------------------------------------------
enum { RING_OK = 0, RING_FAILED = 1, RING_DECLINED = 2 };
bool ring_engaged(const DecodeMode& mode);
// RING_DECLINED: no free slot, or the comparator mode differs from the open batch's - the caller takes the direct path
int ring_call(const DecodeMode& mode, uint32_t framebits, const unsigned int* symbols, unsigned char* out);
// the four vit_set_batch_*: each returns the previous value
int ring_set_window_us(int microseconds);
int ring_set_min_callers(int n);
int ring_set_depth(int launches_in_flight);
int ring_set_spin_cpus(int cpus);
// counts a deconvolve() call (any path) as in flight while it lives
struct RingInflight {
    RingInflight();
    ~RingInflight();
    RingInflight(const RingInflight&) = delete;
    RingInflight& operator=(const RingInflight&) = delete;
};
