// vit_api.hip -- the core of the C ABI of libviterbi.so (include/viterbi_amd.h) and the reference's own exports.
//
// Host side of the drop-in: process state and the device probe, the per-thread HIP stream and staging buffers, the
// fault ("save mode") flag, the call log, and deconvolve / RScheckSuperframe with their batched host-buffer siblings.
// The other units of the C ABI share vit_host.h: vit_ring.hip (the ingest stage for concurrent deconvolve() callers),
// vit_api_decode.hip (kernel choice, the entry points around the decoder) and vit_api_ofdm.hip (the receiver front).
// No decode arithmetic happens on the host; when no gfx950 device is usable every entry point fails loudly with the
// documented error value.
//
// Reference boundary being replaced: viterbi.def:4-8, deconvolve.cpp:551-554,
// rschecksf.cpp:65-93, dllmain.cpp:156-160, setupdll.cpp:195-270 (dispatcher),
// exc_handler.cpp:150-249 (fault -> save mode).
#include <sched.h>

#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>

#include "vit_host.h"

static thread_local char t_err[256] = "";

namespace {

// ---- opt-in call log, the analogue of the reference's VIT_WRITE_LOGFILE build -------------------
// (deconvolve.cpp:568-649, rschecksf.cpp:94-186): VITERBI_AMD_LOG=<path> appends one line per
// exported call: sequence number, wall-clock time, thread id, call, size, duration, return value.
struct CallLog {
    FILE* f = nullptr;
    std::mutex mu;
    std::atomic<unsigned> seq{0};
    CallLog() {
        if (const char* p = getenv("VITERBI_AMD_LOG")) f = fopen(p, "a");
    }
    void line(const char* what, unsigned size, double us, int rc) {
        if (!f) return;
        const auto now = std::chrono::system_clock::now().time_since_epoch();
        const long long usec = std::chrono::duration_cast<std::chrono::microseconds>(now).count();
        std::lock_guard<std::mutex> lk(mu);
        fprintf(f, "%6u  %lld.%06lld  TID: %zu  %s  size: %u  dur: %.1f us  ret: %d\n", seq++, usec / 1000000,
                usec % 1000000, std::hash<std::thread::id>()(std::this_thread::get_id()) % 100000, what, size, us, rc);
        fflush(f);
    }
};
CallLog* g_log = new CallLog();  // never destroyed: calls may come from other threads during exit
struct ScopedCall {
    const char* what; unsigned size; int* rc; std::chrono::steady_clock::time_point t0;
    ScopedCall(const char* w, unsigned s, int* r) : what(w), size(s), rc(r) {
        if (g_log->f) t0 = std::chrono::steady_clock::now();
    }
    ~ScopedCall() {
        if (g_log->f)
            g_log->line(what, size, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(), *rc);
    }
};

// ---- process-wide state (written at init only, like deconJumpTarget) -------
std::once_flag g_once;
int g_ndev = 0;           // usable gfx950 devices
int g_device = -1;        // selected device (host-buffer entry points; *_dev calls use the caller's current device)
int g_cus = 0;
char g_init_err[160] = "no usable gfx950 (MI355X) HIP device; libviterbi has no CPU path";
std::atomic<int> g_fault{0};   // reference: exceptCounter / decon_savemode
std::atomic<int> g_kernel{0};  // 0 auto, 1 wave, 2 packed, 3 latency
// Renormalisation comparator of every decoder kernel: 1 = `>= 150`, the reference's MASM decoders (decon_avx2.asm:97,114
// `cmp sil,150 ; jb mainloop`; configuration Rel_asm - the one the reference's README tells users to build (README.md:50-52),
// i.e. what an installed viterbi.dll runs, and therefore the DEFAULT of this drop-in since round 4); 0 = `> 150`, its C
// decoders (deconvolve.cpp:399,408, configuration Rel_cpp - the one that can be compiled outside Windows and that the
// timed AVX2 port and bench.py's parity check implement).  Environment VITERBI_AMD_RENORM_GE=0/1 sets the start-up value;
// vit_set_renorm_ge() changes it.
std::atomic<int> g_renorm_ge{[] {
    const char* e = getenv("VITERBI_AMD_RENORM_GE");
    return e ? (atoi(e) != 0 ? 1 : 0) : 1;
}()};

void probe_devices() {
    // Callers are threads (README.md:56), each with its own stream.  ROCclr multiplexes a process's streams onto
    // GPU_MAX_HW_QUEUES hardware queues (default 4) and kernels that share a queue run one after the other, so
    // a host with many concurrent deconvolve() callers wants more.  That is the host's policy:
    // the library only touches the environment when VITERBI_AMD_HW_QUEUES explicitly asks it to, and only if this
    // is early enough (before the process's first HIP call) and GPU_MAX_HW_QUEUES is not set already.
    if (const char* q = getenv("VITERBI_AMD_HW_QUEUES"))
        if (atoi(q) > 0) setenv("GPU_MAX_HW_QUEUES", q, 0);
    // The first HIP call of a process can fail transiently right after another process has released the GPU (seen once on a
    // freshly acquired box: torch saw the device, this probe did not).  The probe runs once per process, so it does not give up
    // at the first answer: up to 2 s of retries, and the error text says what HIP reported.
    int n = 0;
    hipError_t pe = hipSuccess;
    for (int attempt = 0; attempt < 20; attempt++) {
        pe = hipGetDeviceCount(&n);
        if (pe == hipSuccess && n > 0) break;
        (void)hipGetLastError();
        n = 0;
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
    }
    if (n <= 0) {
        snprintf(g_init_err, sizeof g_init_err, "no usable gfx950 (MI355X) HIP device (hipGetDeviceCount: %s); libviterbi has no CPU path",
                 pe == hipSuccess ? "0 devices" : hipGetErrorString(pe));
        g_ndev = 0;
        g_device = -1;
        return;
    }
    int want = 0;
    if (const char* e = getenv("VITERBI_AMD_DEVICE")) want = atoi(e);
    int usable = 0, chosen = -1;
    for (int d = 0; d < n; d++) {
        hipDeviceProp_t pr;
        if (hipGetDeviceProperties(&pr, d) != hipSuccess) continue;
        if (strncmp(pr.gcnArchName, "gfx950", 6) != 0) continue;  // kernels exist for gfx950 only
        if (usable == want) { chosen = d; g_cus = pr.multiProcessorCount; }
        usable++;
    }
    g_ndev = usable;
    g_device = chosen;
    if (usable > 0 && chosen < 0)  // never fall back silently to another GPU than the one asked for
        snprintf(g_init_err, sizeof g_init_err, "VITERBI_AMD_DEVICE=%d is out of range: %d usable gfx950 device(s)", want,
                 usable);
}
void ensure_init() { std::call_once(g_once, probe_devices); }

// ---- per-thread context: stream + staging (README.md:56: callers are threads) ----
// Everything in it belongs to ONE device (`dev`).
struct ThreadCtx {
    int dev = -1;
    hipStream_t stream = nullptr;
    void* h_pin = nullptr;   size_t h_cap = 0;   // pinned host staging (mapped: h_pin_dev is its device view)
    void* h_pin_dev = nullptr;
    void* d_in = nullptr;    size_t din_cap = 0; // device input (u32 or u8 / RS block)
    void* d_sym8 = nullptr;  size_t d8_cap = 0;  // packed symbols
    void* d_out = nullptr;   size_t dout_cap = 0;
    void* d_ret = nullptr;   size_t dret_cap = 0;
    void* d_desc = nullptr;  size_t ddesc_cap = 0;  // bounds-checked descriptor copy (vit_decode_varlen_dev_checked)
    hipEvent_t scratch_ev = nullptr;  // last use of d_sym8 / d_desc by a *_dev call on a caller-owned stream
    uint32_t seq = 0;                 // completion sequence number of the single-call latency path
    bool ready = false;
    void release() {
        if (!ready) return;
        // process teardown may already have destroyed the runtime: ignore errors
        if (h_pin) (void)hipHostFree(h_pin);
        if (d_in) (void)hipFree(d_in);
        if (d_sym8) (void)hipFree(d_sym8);
        if (d_out) (void)hipFree(d_out);
        if (d_ret) (void)hipFree(d_ret);
        if (d_desc) (void)hipFree(d_desc);
        if (scratch_ev) (void)hipEventDestroy(scratch_ev);
        if (stream) (void)hipStreamDestroy(stream);
        *this = ThreadCtx();
    }
    ~ThreadCtx() { release(); }
};
// One context per (thread, device): a thread that alternates between devices (vit_decode_stream_multi drives all its
// ranks from one host thread) keeps every device's stream and buffers instead of freeing and re-creating them.
constexpr int VIT_MAX_DEVS = 64;
struct ThreadCtxs {
    ThreadCtx by_dev[VIT_MAX_DEVS];
};
thread_local ThreadCtxs t_ctxs;

// Makes the calling thread's context usable on device `dev`, which must be the CURRENT device (the exported
// entry points hold a VitDeviceGuard, so the caller's own current device is restored when they return).
int ctx_prepare(int dev, ThreadCtx*& ctx) {
    if (dev < 0 || dev >= VIT_MAX_DEVS) return bad_arg("HIP device ordinal %d out of range", dev);
    ctx = &t_ctxs.by_dev[dev];
    if (!ctx->ready) {
        HIPCHK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        ctx->dev = dev;
        ctx->ready = true;
    }
    return VIT_OK;
}
int grow_dev(void** p, size_t* cap, size_t need) {
    if (*cap >= need) return VIT_OK;
    if (*p) HIPCHK(hipFree(*p));
    *p = nullptr; *cap = 0;
    size_t sz = need < 65536 ? 65536 : need + need / 4;
    HIPCHK(hipMalloc(p, sz));
    *cap = sz;
    return VIT_OK;
}
int grow_pin(ThreadCtx& ctx, size_t need) {
    if (ctx.h_cap >= need) return VIT_OK;
    if (ctx.h_pin) HIPCHK(hipHostFree(ctx.h_pin));
    ctx.h_pin = nullptr; ctx.h_pin_dev = nullptr; ctx.h_cap = 0;
    size_t sz = need < 65536 ? 65536 : need + need / 4;
    HIPCHK(hipHostMalloc(&ctx.h_pin, sz, hipHostMallocMapped));
    HIPCHK(hipHostGetDevicePointer(&ctx.h_pin_dev, ctx.h_pin, 0));
    ctx.h_cap = sz;
    return VIT_OK;
}

// Spins until done() holds: the end-of-kernel signal and hipStreamSynchronize's wake-up stay off the call's critical
// path.  A kernel that does not publish within the spin budget (20 ms) falls back to the stream's own completion: its
// error, or hipSuccess with *silent = "the stream completed and done() still does not hold".
template <class Done>
hipError_t spin_until(Done done, hipStream_t stream, bool* silent) {
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    while (!done()) {
        __builtin_ia32_pause();
        if (++spins > 4096u && (spins & 63u) == 0) sched_yield();  // more callers than cores: let the others run
        if ((spins & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) {
            const hipError_t e = hipStreamSynchronize(stream);
            *silent = e == hipSuccess && !done();
            return e;
        }
    }
    return hipSuccess;
}

}  // namespace

int hip_device_ready() {
    ensure_init();
    if (g_device < 0) {
        set_err("%s", g_init_err);
        return VIT_ERR_NO_DEVICE;
    }
    return VIT_OK;
}
int vit_default_device() { return g_device; }
DecodeMode decode_mode() { return DecodeMode{g_kernel.load(), g_renorm_ge.load() != 0}; }
hipStream_t vit_thread_stream(int dev) {
    ThreadCtx* ctx = nullptr;
    return ctx_prepare(dev, ctx) == VIT_OK ? ctx->stream : nullptr;
}

int ScratchLease::begin(size_t sym_bytes, size_t desc_bytes, hipStream_t stream) {
    int dev = -1;
    HIPCHK(hipGetDevice(&dev));
    ThreadCtx* ctx = nullptr;
    int rc = ctx_prepare(dev, ctx);
    if (rc != VIT_OK) return rc;
    if ((rc = grow_dev(&ctx->d_sym8, &ctx->d8_cap, sym_bytes)) != VIT_OK) return rc;
    if ((rc = grow_dev(&ctx->d_desc, &ctx->ddesc_cap, desc_bytes)) != VIT_OK) return rc;
    if (!ctx->scratch_ev) HIPCHK(hipEventCreateWithFlags(&ctx->scratch_ev, hipEventDisableTiming));
    else HIPCHK(hipStreamWaitEvent(stream, ctx->scratch_ev, 0));
    sym_ = ctx->d_sym8;
    desc_ = ctx->d_desc;
    ev_ = ctx->scratch_ev;
    stream_ = stream;
    return VIT_OK;
}
int ScratchLease::end() {
    HIPCHK(hipEventRecord(ev_, stream_));
    return VIT_OK;
}

static void vset_err(const char* fmt, va_list ap) {
    vsnprintf(t_err, sizeof t_err, fmt, ap);
    if (getenv("VITERBI_AMD_VERBOSE")) fprintf(stderr, "[libviterbi] %s\n", t_err);
}
void vit_set_err(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vset_err(fmt, ap);
    va_end(ap);
}
int bad_arg(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vset_err(fmt, ap);
    va_end(ap);
    return VIT_ERR_ARG;
}

int vit_device_cus(int dev) {
    static std::mutex mu;
    static int cus[64] = {0};
    if (dev < 0 || dev >= 64) return 256;
    std::lock_guard<std::mutex> lk(mu);
    if (cus[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev] = n;
    }
    return cus[dev];
}

hipError_t vit_optin_dynamic_lds(const void* const* kernels, int nkernels, int bytes, int dev, uint64_t* done) {
    static std::mutex mu;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lk(mu);
    if ((*done >> dev) & 1u) return hipSuccess;
    for (int i = 0; i < nkernels; i++) {
        const hipError_t e = hipFuncSetAttribute(kernels[i], hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return e;
    }
    *done |= 1ull << dev;
    return hipSuccess;
}

extern "C" {

const char* vit_last_error(void) { return t_err; }

int vit_device_count(void) {
    ensure_init();
    if (g_ndev == 0) set_err("%s", g_init_err);
    return g_ndev;
}

int vit_set_batch_window_us(int microseconds) { return ring_set_window_us(microseconds); }
int vit_set_batch_min_callers(int n) { return ring_set_min_callers(n); }
int vit_set_batch_depth(int launches_in_flight) { return ring_set_depth(launches_in_flight); }
int vit_set_batch_spin_cpus(int cpus) { return ring_set_spin_cpus(cpus); }

int vit_set_kernel(int which) {
    if (which < K_AUTO || which > K_MAX) which = K_AUTO;
    return g_kernel.exchange(which);
}

int vit_set_renorm_ge(int on) { return g_renorm_ge.exchange(on ? 1 : 0); }

unsigned char initialize(void) {
    // dllmain.cpp:156-160: clear the fault counter and re-run the (idempotent) set-up.
    g_fault.store(0);
    ensure_init();
    (void)hipGetLastError();
    return 1;
}

int GetCPUCaps(void) {
    ensure_init();
    if (g_device < 0) return 0;
    return VIT_CAPS_GFX950 | (g_cus << 8);
}

void WakeUpYMM(void) {
    if (hip_device_ready() != VIT_OK) return;
    VitDeviceGuard guard(g_device);
    ThreadCtx* ctx = nullptr;
    if (ctx_prepare(g_device, ctx) != VIT_OK) return;
    (void)grow_pin(*ctx, 65536);
    (void)grow_dev(&ctx->d_in, &ctx->din_cap, 65536);
    (void)grow_dev(&ctx->d_sym8, &ctx->d8_cap, 65536);
    (void)grow_dev(&ctx->d_out, &ctx->dout_cap, 65536);
}

int vit_decode_batch_host(const uint8_t* h_symbols_u8, uint8_t* h_decoded, uint32_t framebits, int64_t nframes) {
    if (!valid_framebits(framebits) || nframes < 0 || (nframes > 0 && framebits > 0 && (!h_symbols_u8 || !h_decoded)))
        return bad_arg("vit_decode_batch_host: bad arguments");
    if (framebits == 0 || nframes == 0) return VIT_OK;
    int rc = hip_device_ready();
    if (rc != VIT_OK) return rc;
    VitDeviceGuard guard(g_device);
    ThreadCtx* ctx = nullptr;
    if ((rc = ctx_prepare(g_device, ctx)) != VIT_OK) return rc;
    const size_t in_sz = (size_t)nframes * 4u * (framebits + VIT_TAIL);
    const size_t out_sz = (size_t)nframes * ((framebits + 7u) >> 3);
    if ((rc = grow_dev(&ctx->d_sym8, &ctx->d8_cap, in_sz)) != VIT_OK) return rc;
    if ((rc = grow_dev(&ctx->d_out, &ctx->dout_cap, out_sz)) != VIT_OK) return rc;
    HIPCHK(hipMemcpyAsync(ctx->d_sym8, h_symbols_u8, in_sz, hipMemcpyHostToDevice, ctx->stream));
    rc = launch_decode(decode_mode(), ctx->d_sym8, false, (uint8_t*)ctx->d_out, nullptr, framebits, framebits,
                       nframes, ctx->stream);
    if (rc != VIT_OK) return rc;
    HIPCHK(hipMemcpyAsync(h_decoded, ctx->d_out, out_sz, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return VIT_OK;
}

static int deconvolve_impl(unsigned int framebits, unsigned int* symbols, unsigned char* decodedBits);
int deconvolve(unsigned int framebits, unsigned int* symbols, int unused, unsigned char* decodedBits) {
    (void)unused;  // never read by the reference either (deconvolve.cpp:447-526)
    int rc = 1;
    ScopedCall log("deconvolve", framebits, &rc);
    rc = deconvolve_impl(framebits, symbols, decodedBits);
    return rc;
}
static int deconvolve_impl(unsigned int framebits, unsigned int* symbols, unsigned char* decodedBits) {
    if (framebits == 0) return 0;  // C path: loop count 0, no memory touched
    if (g_fault.load()) return 1;  // save mode until initialize() (exc_handler.cpp:214,243)
    if (!symbols || !decodedBits || !valid_framebits(framebits)) {
        set_err("deconvolve: bad arguments (framebits=%u)", framebits);
        return 1;
    }
    if (hip_device_ready() != VIT_OK) return 1;
    RingInflight inflight;
    const DecodeMode mode = decode_mode();
    if (ring_engaged(mode)) {  // ingest stage: share a launch with the other callers in flight
        const int r = ring_call(mode, framebits, symbols, decodedBits);
        if (r == RING_OK) return 0;
        if (r == RING_FAILED) {
            g_fault.store(1);
            return 1;
        }
        // declined (no free slot, comparator mode differs from the open batch's): the direct path below
    }
    VitDeviceGuard guard(g_device);
    ThreadCtx* ctx = nullptr;
    if (ctx_prepare(g_device, ctx) != VIT_OK) return 1;
    const size_t nsym = 4u * ((size_t)framebits + VIT_TAIL);
    const size_t out_sz = (framebits + 7u) >> 3;
    const size_t out_off = (nsym + 15u) & ~(size_t)15u;
    const size_t flag_off = (out_off + out_sz + 63u) & ~(size_t)63u;
    if (grow_pin(*ctx, flag_off + 64) != VIT_OK) {
        g_fault.store(1);
        return 1;
    }
    auto fail = [&](const char* what, hipError_t e) {
        set_err("deconvolve: %s: %s", what, hipGetErrorString(e));
        g_fault.store(1);
        return 1;
    };
    // Zero-copy staging: the pinned buffer is mapped into the device's address space.  The caller's u32 symbols are
    // narrowed to the device format (one byte each, the low byte: deconvolve.cpp:158-165) while they are copied into
    // it; the decode kernel reads those 3 KB (FIC) straight from host memory, in one batch of loads, and writes its
    // (framebits+7)/8 bytes straight back: no hipMemcpy round trips, ONE launch, one wait.
    unsigned char* h_out = (unsigned char*)ctx->h_pin + out_off;
    narrow_symbols(symbols, (uint8_t*)ctx->h_pin, nsym);
    hipError_t e;
    if (pick_kernel(mode.kernel, framebits, 1) == K_LATENCY) {
        // Latency path: the kernel publishes a sequence number in the mapped buffer after its last output byte and
        // this thread spins on it - the end-of-kernel signal and hipStreamSynchronize's wake-up are off the call's
        // critical path.  A kernel that does not finish within the spin budget falls back to the stream sync.
        volatile uint32_t* h_flag = reinterpret_cast<volatile uint32_t*>((unsigned char*)ctx->h_pin + flag_off);
        const uint32_t seq = ++ctx->seq ? ctx->seq : ++ctx->seq;  // never 0
        *h_flag = 0;
        e = vit_launch_lat(ctx->h_pin_dev, false, (uint8_t*)ctx->h_pin_dev + out_off, nullptr, framebits, framebits, 1,
                           ctx->stream, reinterpret_cast<uint32_t*>((unsigned char*)ctx->h_pin_dev + flag_off), seq, mode.ge);
        if (e != hipSuccess) return fail("launch", e);
        bool silent = false;
        e = spin_until([&] { return __atomic_load_n(const_cast<uint32_t*>(h_flag), __ATOMIC_ACQUIRE) == seq; }, ctx->stream, &silent);
        if (e != hipSuccess) return fail("sync", e);
        if (silent) {
            set_err("deconvolve: the kernel ended without publishing its result");
            g_fault.store(1);
            return 1;
        }
        memcpy(decodedBits, h_out, out_sz);
        return 0;
    }
    if (launch_decode(mode, ctx->h_pin_dev, false, (uint8_t*)ctx->h_pin_dev + out_off, nullptr, framebits, framebits, 1,
                      ctx->stream) != VIT_OK) {
        g_fault.store(1);
        return 1;
    }
    if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return fail("sync", e);
    memcpy(decodedBits, h_out, out_sz);
    return 0;
}

int vit_rs_batch_host(const uint8_t* h_p, uint8_t* h_out, int32_t* h_ret, uint32_t RSDims, int64_t nsf) {
    if (nsf < 0 || RSDims > 65535u || (nsf > 0 && (!h_ret || (RSDims > 0 && (!h_p || !h_out)))))
        return bad_arg("vit_rs_batch_host: bad arguments");
    if (nsf == 0) return VIT_OK;
    if (RSDims == 0) { memset(h_ret, 0, (size_t)nsf * sizeof(int32_t)); return VIT_OK; }
    int rc = hip_device_ready();
    if (rc != VIT_OK) return rc;
    VitDeviceGuard guard(g_device);
    ThreadCtx* ctx = nullptr;
    if ((rc = ctx_prepare(g_device, ctx)) != VIT_OK) return rc;
    const size_t in_sz = (size_t)nsf * 120u * RSDims, out_sz = (size_t)nsf * 110u * RSDims;
    if ((rc = grow_dev(&ctx->d_in, &ctx->din_cap, in_sz)) != VIT_OK) return rc;
    if ((rc = grow_dev(&ctx->d_out, &ctx->dout_cap, out_sz)) != VIT_OK) return rc;
    if ((rc = grow_dev(&ctx->d_ret, &ctx->dret_cap, (size_t)nsf * 4)) != VIT_OK) return rc;
    HIPCHK(hipMemcpyAsync(ctx->d_in, h_p, in_sz, hipMemcpyHostToDevice, ctx->stream));
    // columns at/after the first failure must keep the caller's bytes: seed the device copy
    HIPCHK(hipMemcpyAsync(ctx->d_out, h_out, out_sz, hipMemcpyHostToDevice, ctx->stream));
    LAUNCHCHK("rs launch failed: %s",
              rs_launch((const uint8_t*)ctx->d_in, (uint8_t*)ctx->d_out, (int32_t*)ctx->d_ret, RSDims, nsf, ctx->stream));
    HIPCHK(hipMemcpyAsync(h_out, ctx->d_out, out_sz, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(h_ret, ctx->d_ret, (size_t)nsf * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return VIT_OK;
}

static int rscheck_impl(unsigned char* p, unsigned int RSDims, unsigned char* outVector);
int RScheckSuperframe(unsigned char* p, int startIx, unsigned int RSDims, unsigned char* outVector) {
    (void)startIx;  // rschecksf.cpp:69
    int rc = -1;
    ScopedCall log("RScheckSuperframe", RSDims, &rc);
    rc = rscheck_impl(p, RSDims, outVector);
    return rc;
}
static int rscheck_impl(unsigned char* p, unsigned int RSDims, unsigned char* outVector) {
    if (RSDims == 0) return 0;
    if (g_fault.load()) return -1;
    if (!p || !outVector || RSDims > 65535u) {
        set_err("RScheckSuperframe: bad arguments");
        return -1;
    }
    // Zero-copy like deconvolve(): the 120*RSDims input bytes, the caller's current output bytes (columns at
    // and after the first failure must keep them) and the return value live in the thread's mapped pinned
    // buffer; the kernel reads and writes host memory directly - one launch, one sync, no hipMemcpy.
    if (hip_device_ready() != VIT_OK) return -1;
    VitDeviceGuard guard(g_device);
    ThreadCtx* ctx = nullptr;
    if (ctx_prepare(g_device, ctx) != VIT_OK) return -1;
    const size_t in_sz = 120u * (size_t)RSDims, out_sz = 110u * (size_t)RSDims;
    const size_t in_pad = (in_sz + 15u) & ~(size_t)15u, out_pad = (out_sz + 15u) & ~(size_t)15u;
    if (grow_pin(*ctx, in_pad + out_pad + 64) != VIT_OK) {
        g_fault.store(1);
        return -1;
    }
    unsigned char* h = (unsigned char*)ctx->h_pin;
    unsigned char* d = (unsigned char*)ctx->h_pin_dev;
    memcpy(h, p, in_sz);
    memcpy(h + in_pad, outVector, out_sz);
    int32_t* h_ret = reinterpret_cast<int32_t*>(h + in_pad + out_pad);
    constexpr int32_t PENDING = 0x7FFFFFFF;  // never a return value: those are -1 or a root count
    const bool poll = RSDims <= 256u;      // the one-workgroup kernel publishes the return value last (see rs_kernel)
    *h_ret = poll ? PENDING : -1;
    hipError_t e = rs_launch(d, d + in_pad, reinterpret_cast<int32_t*>(d + in_pad + out_pad), RSDims, 1, ctx->stream, poll);
    if (e == hipSuccess && poll) {
        bool silent = false;
        e = spin_until([&] { return __atomic_load_n(h_ret, __ATOMIC_ACQUIRE) != PENDING; }, ctx->stream, &silent);
        if (e == hipSuccess && silent) e = hipErrorUnknown;
    } else if (e == hipSuccess) {
        e = hipStreamSynchronize(ctx->stream);
    }
    if (e != hipSuccess) {
        set_err("RScheckSuperframe: %s", hipGetErrorString(e));
        g_fault.store(1);
        return -1;
    }
    memcpy(outVector, h + in_pad, out_sz);
    return *h_ret;
}

int RSCheckSuperframe(unsigned char* p, int startIx, unsigned int RSDims, unsigned char* outVector) {
    return RScheckSuperframe(p, startIx, RSDims, outVector);
}

}  // extern "C"
