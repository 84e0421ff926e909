// vit_ring.hip -- the ingest stage of the C ABI: concurrent deconvolve() callers share launches.
// deconvolve() (vit_api.hip) reaches it through the small interface at the end of this file (vit_host.h).
#include <linux/futex.h>
#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <climits>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "vit_host.h"

namespace {

// ---- ingest stage: concurrent deconvolve() callers share launches ------------------
// The reference is re-entrant and QIRX calls it from several threads (README.md:56).  One call is one 774-step
// dependent chain on one wavefront (~35 us) however empty the GPU is, and a process's streams share a handful of
// hardware queues, so separate launches of concurrent callers queue up behind each other.  The stage:
//
//   * ONE mapped pinned buffer cut into slots.  A caller claims a slot, copies its OWN symbols into it - narrowing
//     the reference ABI's u32 to the device format's one byte per symbol on the way (low byte, deconvolve.cpp:158-165:
//     a quarter of the PCIe traffic) - and spins on the slot's completion word.  Callers copy in parallel; there is
//     no worker thread, no H2D/D2H copy, no descriptor table in memory, no condition variable.
//   * The first caller to arrive while no batch is open becomes that batch's LEADER: it holds the batch open until
//     one of `depth` launch credits is free (i.e. while `depth` earlier batches are still on the GPU, at most
//     `window` microseconds), closes it, and issues ONE bounded launch of the latency kernel with grid = members
//     (vit_lat_ring_kernel: the slot table travels by value in the kernel arguments).  Batches therefore form
//     exactly when launches would otherwise queue: a lone caller finds a credit and launches at once.
//   * Every workgroup publishes the batch's sequence number in its slot's completion word after its last output
//     byte (system-scope release); the caller copies its bytes out and frees the slot.
struct SpinLock {  // test-and-test-and-set; held for a few dozen instructions (join / close a batch)
    std::atomic<int> f{0};
    void lock() {
        for (unsigned n = 1;; n++) {
            if (f.load(std::memory_order_relaxed) == 0 && f.exchange(1, std::memory_order_acquire) == 0) return;
            __builtin_ia32_pause();
            if ((n & 1023u) == 0) sched_yield();  // the holder may have lost its core
        }
    }
    void unlock() { f.store(0, std::memory_order_release); }
};

constexpr uint32_t RING_SLOTS = VIT_RING_MAXB;   // concurrent callers the ring serves; further ones take the direct path
constexpr uint32_t RING_SYM_CAP = 36992;         // >= 4 * (9216 + 6) one-byte symbols
constexpr uint32_t RING_OUT_OFF = RING_SYM_CAP;  // 1152 output bytes
constexpr uint32_t RING_FLAG_OFF = RING_OUT_OFF + 1152;  // completion word, on a cache line of its own
constexpr uint32_t RING_STRIDE = 38400;
static_assert(RING_SYM_CAP >= 4 * (VIT_MAX_FRAMEBITS + VIT_TAIL) && RING_FLAG_OFF % 64 == 0 && RING_FLAG_OFF + 64 <= RING_STRIDE &&
              RING_STRIDE % 128 == 0, "ring slot layout");
constexpr int RING_MAX_DEPTH = 16;

long futex_wait(std::atomic<uint32_t>* a, uint32_t expected, long timeout_ns) {
    timespec ts{0, timeout_ns};
    return syscall(SYS_futex, reinterpret_cast<uint32_t*>(a), FUTEX_WAIT_PRIVATE, expected, &ts, nullptr, 0);
}
void futex_wake_all(std::atomic<uint32_t>* a) {
    (void)syscall(SYS_futex, reinterpret_cast<uint32_t*>(a), FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
}
// CPUs this process may keep busy: the affinity mask, capped by a cgroup CPU quota (a container that may use 16 CPUs'
// worth of time on a 256-CPU host is THROTTLED when 32 threads spin).  Waiting callers spin only while the calls in
// flight fit this budget; beyond it all but one per batch sleep on a futex.
int detect_cpu_budget() {
    cpu_set_t set;
    int n = sched_getaffinity(0, sizeof set, &set) == 0 ? CPU_COUNT(&set) : 1;
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota|max> <period>"
        char q[32] = "";
        long period = 0;
        if (fscanf(f, "%31s %ld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
            const long cpus = (atol(q) + period - 1) / period;
            if (cpus > 0 && cpus < n) n = (int)cpus;
        }
        fclose(f);
    } else {
        long quota = -1, period = 0;  // cgroup v1
        if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(g, "%ld", &quota) != 1) quota = -1; fclose(g); }
        if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(g, "%ld", &period) != 1) period = 0; fclose(g); }
        if (quota > 0 && period > 0 && (quota + period - 1) / period < n) n = (int)((quota + period - 1) / period);
    }
    return n < 1 ? 1 : n;
}

// VITERBI_AMD_RING_STATS=1: where a call's time goes, printed to stderr (and reset) by every vit_set_batch_window_us() call
struct RingStats {
    const bool on = getenv("VITERBI_AMD_RING_STATS") != nullptr;
    std::atomic<uint64_t> calls{0}, batches{0}, declined{0}, ns_call{0}, ns_copy{0}, ns_token{0}, ns_members{0}, ns_launch{0},
        ns_leader_wait{0}, ns_follower_wait{0}, ns_wake_delay{0}, wakes{0}, slept{0}, takeovers{0}, no_token{0};
    static uint64_t now() {
        return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }
    void print_and_reset() {
        const uint64_t c = calls.exchange(0), b = batches.exchange(0);
        if (c && b)
            fprintf(stderr,
                    "[ring] calls %llu batches %llu (%.1f per batch) declined %llu | per call: total %.1f us copy %.1f | per batch: token wait %.1f "
                    "members' copies %.1f launch call %.1f leader wait %.1f | followers: wait %.1f us, slept %llu, wake delay %.1f us (%llu), "
                    "poller take-overs %llu, launches without token %llu\n",
                    (unsigned long long)c, (unsigned long long)b, (double)c / b, (unsigned long long)declined.load(), ns_call.load() / 1e3 / c,
                    ns_copy.load() / 1e3 / c, ns_token.load() / 1e3 / b, ns_members.load() / 1e3 / b, ns_launch.load() / 1e3 / b,
                    ns_leader_wait.load() / 1e3 / b, c > b ? ns_follower_wait.load() / 1e3 / (c - b) : 0.0, (unsigned long long)slept.load(),
                    wakes.load() ? ns_wake_delay.load() / 1e3 / wakes.load() : 0.0, (unsigned long long)wakes.load(),
                    (unsigned long long)takeovers.load(), (unsigned long long)no_token.load());
        for (auto* a : {&declined, &ns_call, &ns_copy, &ns_token, &ns_members, &ns_launch, &ns_leader_wait, &ns_follower_wait, &ns_wake_delay,
                        &wakes, &slept, &takeovers, &no_token})
            a->store(0);
    }
};
RingStats g_rstat;

struct RingBatch {
    VitRingTable tbl;                  // members (what the kernel receives by value)
    uint32_t maxfb = 0;
    bool ge = false;
    int token = -1;                    // launch token (= index of the ring stream) the leader holds, -1: none
    hipStream_t stream = nullptr;      // the stream the batch was launched on
    std::atomic<uint32_t> copied{0};   // members whose symbols are in their slot
    std::atomic<int> state{0};         // 0 not launched yet, 1 launched, 2 failed before the launch, 3 failed after it
    std::atomic<uint32_t> refs{0};     // members that have not left yet
    // waiting: ONE member at a time (the leader first) is the batch's poller: it spins on the completion words and
    // wakes the members that sleep; the others spin on their own word while CPUs are to spare, or sleep
    std::atomic<int> poller{0};                        // 1 while a member polls for the others
    std::atomic<uint32_t> wake[VIT_RING_MAXB];         // per member futex word: 0 = must wait, WAKE_DONE, WAKE_POLL
    std::atomic<uint8_t> asleep[VIT_RING_MAXB];        // member sleeps (or is about to) on its futex word
    std::atomic<uint8_t> gone[VIT_RING_MAXB];          // member has seen its own completion (its slot may be reused)
    std::atomic<uint64_t> t_seen[VIT_RING_MAXB];       // statistics only: when the poller saw the member's completion
};
enum : uint32_t { WAKE_DONE = 1, WAKE_POLL = 2 };
struct Ring {
    SpinLock mu;                       // joining and closing the open batch; everything else is lock-free
    std::once_flag once;
    int init_rc = VIT_ERR_HIP;
    uint8_t* h_base = nullptr;
    uint8_t* d_base = nullptr;
    // free slots / batch records: bit masks; claimed under `mu` (one claimer at a time), released with one atomic OR
    std::atomic<uint64_t> slot_free[2] = {};
    std::atomic<uint64_t> batch_free[2] = {};
    RingBatch batches[RING_SLOTS];     // every live batch has a member holding a slot: never more than RING_SLOTS
    RingBatch* open = nullptr;         // the batch a new caller joins (under mu)
    uint32_t seq = 0;
    // launch tokens: token i = the right to have one batch in flight on streams[i].  Batches in flight therefore never
    // share a stream (streams of arbitrary caller threads would: a process's streams are multiplexed onto a few
    // hardware queues, and two batches on one queue run one after the other).
    hipStream_t streams[RING_MAX_DEPTH] = {};
    std::atomic<uint32_t> token_free{(1u << RING_MAX_DEPTH) - 1u};
    std::atomic<int> depth{4};         // batches in flight
    std::atomic<int> window_us{50};    // 0 = stage off
    std::atomic<int> min_callers{1};   // engage only while at least this many deconvolve() calls are in flight
    std::atomic<int> inflight{0};      // deconvolve() calls currently executing (any path)
    std::atomic<int> spin_cpus{0};     // waiting callers spin while the calls in flight do not exceed this

    Ring() {
        // a host that only binds the five reference exports configures the stage through the environment
        // (the analogue of the reference's viterbi.txt)
        if (const char* e = getenv("VITERBI_AMD_BATCH_WINDOW_US")) {
            const int w = atoi(e);
            window_us.store(w < 0 ? 0 : w > 100000 ? 100000 : w);
        }
        if (const char* e = getenv("VITERBI_AMD_BATCH_MIN_CALLERS")) {
            const int n = atoi(e);
            min_callers.store(n < 1 ? 1 : n);
        }
        if (const char* e = getenv("VITERBI_AMD_BATCH_DEPTH")) set_depth(atoi(e));
        // waiting callers spin only while the calls in flight use at most a quarter of the process's CPU budget
        // (profiles/r04_vitbench_sweep.txt: spinning up to the whole budget throttles a quota-limited container)
        const char* e = getenv("VITERBI_AMD_SPIN_CPUS");
        spin_cpus.store(e ? (atoi(e) < 0 ? 0 : atoi(e)) : detect_cpu_budget() / 4);
    }
    int set_depth(int n) { return depth.exchange(n < 1 ? 1 : n > RING_MAX_DEPTH ? RING_MAX_DEPTH : n); }
    int take_token() {  // -1: `depth` batches are in flight
        uint32_t f = token_free.load(std::memory_order_relaxed);
        for (;;) {
            if (RING_MAX_DEPTH - __builtin_popcount(f) >= depth.load(std::memory_order_relaxed) || f == 0) return -1;
            const int t = __builtin_ctz(f);
            if (token_free.compare_exchange_weak(f, f & ~(1u << t), std::memory_order_acquire)) return t;
        }
    }
    static int claim_bit(std::atomic<uint64_t> (&m)[2]) {  // under mu; -1: none
        for (int w = 0; w < 2; w++) {
            const uint64_t v = m[w].load(std::memory_order_acquire);
            if (v) {
                const int bit = __builtin_ctzll(v);
                m[w].fetch_and(~(1ull << bit), std::memory_order_acquire);
                return w * 64 + bit;
            }
        }
        return -1;
    }
    static void free_bit(std::atomic<uint64_t> (&m)[2], uint32_t i) { m[i >> 6].fetch_or(1ull << (i & 63u), std::memory_order_release); }
    void allocate() {
        VitDeviceGuard guard(vit_default_device());
        void* h = nullptr;
        void* d = nullptr;
        if (hipHostMalloc(&h, (size_t)RING_SLOTS * RING_STRIDE, hipHostMallocMapped) != hipSuccess ||
            hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
            (void)hipGetLastError();
            if (h) (void)hipHostFree(h);
            return;
        }
        for (int i = 0; i < RING_MAX_DEPTH; i++)
            if (hipStreamCreateWithFlags(&streams[i], hipStreamNonBlocking) != hipSuccess) {
                (void)hipGetLastError();
                return;
            }
        h_base = (uint8_t*)h;
        d_base = (uint8_t*)d;
        for (uint32_t i = 0; i < RING_SLOTS; i++) {
            batches[i].tbl.stride = RING_STRIDE;
            batches[i].tbl.out_off = RING_OUT_OFF;
            batches[i].tbl.flag_off = RING_FLAG_OFF;
        }
        static_assert(RING_SLOTS == 128, "two 64-bit masks");
        slot_free[0] = slot_free[1] = batch_free[0] = batch_free[1] = ~0ull;
        init_rc = VIT_OK;
    }
    bool engaged(const DecodeMode& mode) {
        if (window_us.load(std::memory_order_relaxed) <= 0) return false;
        if (mode.kernel != K_AUTO && mode.kernel != K_LATENCY) return false;  // a forced kernel keeps the direct path
        return inflight.load(std::memory_order_relaxed) >= min_callers.load(std::memory_order_relaxed);
    }
    uint32_t* flag_of(uint32_t slot) { return reinterpret_cast<uint32_t*>(h_base + (size_t)slot * RING_STRIDE + RING_FLAG_OFF); }
    int call(const DecodeMode& mode, uint32_t framebits, const unsigned int* symbols, unsigned char* out);
    int wait_done(RingBatch* b, uint32_t idx, uint32_t* flag, uint32_t my_seq, bool leader);
};
Ring* g_ring = new Ring();  // intentionally never destroyed (calls may come from other threads during exit)

// Waits until this member's completion word carries the batch's sequence number.  Returns RING_OK / RING_FAILED.
int Ring::wait_done(RingBatch* b, uint32_t idx, uint32_t* flag, uint32_t my_seq, bool leader) {
    auto mine_done = [&] { return __atomic_load_n(flag, __ATOMIC_ACQUIRE) == my_seq; };
    const auto t0 = std::chrono::steady_clock::now();
    bool synced = false;
    // Every few hundred iterations: has the launch failed, is it overdue?  (true = give up)
    auto overdue = [&]() -> bool {
        if (b->state.load(std::memory_order_acquire) >= 2) return !mine_done();
        const auto waited = std::chrono::steady_clock::now() - t0;
        if (leader && !synced && waited > std::chrono::milliseconds(20)) {
            // not what a healthy launch does: fall back to the stream's own completion, once
            const hipError_t e = b->stream ? hipStreamSynchronize(b->stream) : hipErrorUnknown;
            synced = true;
            if (e != hipSuccess || !mine_done()) {
                set_err("deconvolve: the batch launch did not complete (%s)", hipGetErrorString(e));
                b->state.store(3, std::memory_order_release);
                return true;
            }
        } else if (waited > std::chrono::seconds(10)) {
            set_err("deconvolve: no completion from the batch launch");
            b->state.store(3, std::memory_order_release);
            return true;
        }
        return false;
    };
    auto wake_member = [&](uint32_t i, uint32_t what) {
        b->wake[i].store(what, std::memory_order_seq_cst);
        if (b->asleep[i].load(std::memory_order_seq_cst))
            (void)syscall(SYS_futex, reinterpret_cast<uint32_t*>(&b->wake[i]), FUTEX_WAKE_PRIVATE, 1, nullptr, nullptr, 0);
    };
    // This member leaves (or failed): if others still wait asleep, ONE of them must poll from here on.
    auto pass_on = [&] {
        const uint32_t n = b->tbl.n;
        for (uint32_t i = 0; i < n; i++) {
            if (i == idx || b->gone[i].load(std::memory_order_relaxed)) continue;
            if (__atomic_load_n(flag_of(b->tbl.slot[i]), __ATOMIC_RELAXED) == my_seq) { wake_member(i, WAKE_DONE); continue; }
            if (b->asleep[i].load(std::memory_order_seq_cst)) { wake_member(i, WAKE_POLL); return; }
        }
    };
    bool polling = leader;  // the leader has taken the poller's role before the launch
    bool seen[VIT_RING_MAXB];
    for (;;) {
        if (polling) {
            // ---- poller: watch every member's word, wake the sleeper whose frame is done ----
            const uint32_t n = b->tbl.n;  // final: the batch was closed before its launch, and only a launched batch is polled
            for (uint32_t i = 0; i < n; i++) seen[i] = i == idx;
            uint32_t left = n - 1;
            for (unsigned it = 1;; it++) {
                for (uint32_t i = 0; i < n && left; i++) {
                    if (seen[i]) continue;
                    if (b->gone[i].load(std::memory_order_relaxed)) { seen[i] = true; left--; continue; }
                    if (__atomic_load_n(flag_of(b->tbl.slot[i]), __ATOMIC_RELAXED) == my_seq) {
                        seen[i] = true;
                        left--;
                        if (g_rstat.on) b->t_seen[i].store(RingStats::now(), std::memory_order_relaxed);
                        wake_member(i, WAKE_DONE);
                    }
                }
                const bool failed = (it & 255u) == 0 && overdue();
                if (mine_done() || failed) {
                    // hand the role to a member that still waits asleep (a spinning one needs nobody)
                    b->poller.store(0, std::memory_order_seq_cst);
                    if (failed) {
                        for (uint32_t i = 0; i < n; i++)
                            if (!seen[i]) wake_member(i, WAKE_DONE);  // they find the batch's state themselves
                    } else if (left) {
                        pass_on();
                    }
                    return failed ? RING_FAILED : RING_OK;
                }
                __builtin_ia32_pause();
            }
        }
        // ---- not the poller: spin on the own word while CPUs are to spare, else sleep until the poller wakes us ----
        if (inflight.load(std::memory_order_relaxed) <= spin_cpus.load(std::memory_order_relaxed)) {
            for (unsigned it = 1; !mine_done(); it++) {
                __builtin_ia32_pause();
                if ((it & 255u) == 0) {
                    if (overdue()) return RING_FAILED;
                    if (inflight.load(std::memory_order_relaxed) > spin_cpus.load(std::memory_order_relaxed)) break;  // crowded now
                }
            }
            if (mine_done()) return RING_OK;
        }
        b->asleep[idx].store(1, std::memory_order_seq_cst);
        const uint32_t w = b->wake[idx].load(std::memory_order_seq_cst);
        if (mine_done()) {
            if (w == WAKE_POLL) pass_on();  // asked to poll, but already done
            return RING_OK;
        }
        int expect = 0;
        if (w == WAKE_POLL ||
            (b->state.load(std::memory_order_acquire) == 1 && b->poller.load(std::memory_order_seq_cst) == 0 &&
             b->poller.compare_exchange_strong(expect, 1, std::memory_order_seq_cst))) {
            if (w == WAKE_POLL) b->poller.store(1, std::memory_order_seq_cst);
            b->wake[idx].store(0, std::memory_order_relaxed);
            b->asleep[idx].store(0, std::memory_order_seq_cst);
            polling = true;  // the poller has left with its own frame done: this member polls from here on
            if (g_rstat.on) g_rstat.takeovers++;
            continue;
        }
        if (w == 0) {
            if (g_rstat.on) g_rstat.slept++;
            futex_wait(&b->wake[idx], 0, 2000000);  // 2 ms: a missed wake-up costs time, never the result
        }
        if (mine_done()) {
            if (g_rstat.on) {
                const uint64_t ts = b->t_seen[idx].load(std::memory_order_relaxed);
                if (ts) { g_rstat.ns_wake_delay += RingStats::now() - ts; g_rstat.wakes++; }
            }
            if (b->wake[idx].load(std::memory_order_seq_cst) == WAKE_POLL) pass_on();
            return RING_OK;
        }
        if (overdue()) return RING_FAILED;
    }
}

int Ring::call(const DecodeMode& mode, uint32_t framebits, const unsigned int* symbols, unsigned char* out) {
    std::call_once(once, [this] { allocate(); });
    if (init_rc != VIT_OK) return RING_DECLINED;
    const bool st = g_rstat.on;
    const uint64_t t_in = st ? RingStats::now() : 0;
    // ---- join the open batch, or open one ----
    mu.lock();
    RingBatch* b = open;
    const int slot_i = (b && b->ge != mode.ge) ? -1 : claim_bit(slot_free);
    if (slot_i < 0) {
        mu.unlock();
        if (st) g_rstat.declined++;
        return RING_DECLINED;
    }
    const uint32_t slot = (uint32_t)slot_i;
    const bool leader = b == nullptr;
    if (leader) {
        b = &batches[claim_bit(batch_free)];  // never fails: a live batch holds a slot, and there are as many records as slots
        b->tbl.n = 0;
        if (++seq == 0) ++seq;
        b->tbl.seq = seq;
        b->maxfb = 0;
        b->ge = mode.ge;
        b->token = -1;
        b->stream = nullptr;
        b->copied.store(0, std::memory_order_relaxed);
        b->state.store(0, std::memory_order_relaxed);
        b->refs.store(0, std::memory_order_relaxed);
        b->poller.store(1, std::memory_order_relaxed);  // the leader
        open = b;
    }
    const uint32_t idx = b->tbl.n++;
    b->tbl.slot[idx] = (uint16_t)slot;
    b->tbl.fb[idx] = (uint16_t)framebits;
    b->gone[idx].store(0, std::memory_order_relaxed);
    b->asleep[idx].store(0, std::memory_order_relaxed);
    b->wake[idx].store(0, std::memory_order_relaxed);
    b->t_seen[idx].store(0, std::memory_order_relaxed);
    if (framebits > b->maxfb) b->maxfb = framebits;
    b->refs.fetch_add(1, std::memory_order_relaxed);
    if (b->tbl.n == VIT_RING_MAXB) open = nullptr;
    const uint32_t my_seq = b->tbl.seq;
    mu.unlock();

    // ---- the caller's own copy, in parallel with everybody else's ----
    uint8_t* hs = h_base + (size_t)slot * RING_STRIDE;
    uint32_t* flag = flag_of(slot);
    __atomic_store_n(flag, 0u, __ATOMIC_RELAXED);
    narrow_symbols(symbols, hs, 4u * ((size_t)framebits + VIT_TAIL));
    b->copied.fetch_add(1, std::memory_order_release);
    const uint64_t t_copied = st ? RingStats::now() : 0;
    uint64_t t_wait0 = t_copied;

    if (leader) {
        // hold the batch open while `depth` launches are in flight (bounded by the window), then close it
        const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(window_us.load(std::memory_order_relaxed));
        int token = -1;
        for (unsigned spins = 1; (token = take_token()) < 0; spins++) {
            __builtin_ia32_pause();
            if ((spins & 31u) == 0 && std::chrono::steady_clock::now() > deadline) break;
        }
        const uint64_t t_tok = st ? RingStats::now() : 0;
        mu.lock();
        if (open == b) open = nullptr;
        const uint32_t n = b->tbl.n;
        mu.unlock();
        for (unsigned spins = 1; b->copied.load(std::memory_order_acquire) < n; spins++) {  // members still copying
            __builtin_ia32_pause();
            if ((spins & 1023u) == 0) sched_yield();
        }
        const uint64_t t_mem = st ? RingStats::now() : 0;
        hipError_t e = hipErrorUnknown;
        {
            const int dev = vit_default_device();
            VitDeviceGuard guard(dev);
            hipStream_t s = token >= 0 ? streams[token] : vit_thread_stream(dev);  // the window ran out: one launch beyond `depth`, on this thread's stream
            if (s) {
                b->token = token;
                b->stream = s;
                e = vit_launch_lat_ring(d_base, b->tbl, b->maxfb, s, b->ge);
                (void)launch_ok("deconvolve: batch launch: %s", e);
            }
        }
        b->state.store(e == hipSuccess ? 1 : 2, std::memory_order_release);
        if (st) {
            t_wait0 = RingStats::now();
            g_rstat.batches++;
            g_rstat.ns_token += t_tok - t_copied;
            g_rstat.ns_members += t_mem - t_tok;
            g_rstat.ns_launch += t_wait0 - t_mem;
            if (token < 0) g_rstat.no_token++;
        }
        if (e != hipSuccess)  // nobody will ever be woken by a completion word
            for (uint32_t i = 0; i < n; i++)
                if (i != idx) {
                    b->wake[i].store(WAKE_DONE, std::memory_order_seq_cst);
                    (void)syscall(SYS_futex, reinterpret_cast<uint32_t*>(&b->wake[i]), FUTEX_WAKE_PRIVATE, 1, nullptr, nullptr, 0);
                }
    }

    const int rc = wait_done(b, idx, flag, my_seq, leader);
    if (rc == RING_OK) memcpy(out, hs + RING_OUT_OFF, (framebits + 7u) >> 3);
    else if (!leader) set_err("deconvolve: the shared launch failed");
    if (st) {
        const uint64_t t_out = RingStats::now();
        g_rstat.calls++;
        g_rstat.ns_call += t_out - t_in;
        g_rstat.ns_copy += t_copied - t_in;
        (leader ? g_rstat.ns_leader_wait : g_rstat.ns_follower_wait) += t_out - t_wait0;
    }
    // ---- leave: no lock ----
    // the leader's frame is done: its launch has at least started to retire, the next batch may go
    if (leader && b->token >= 0) token_free.fetch_or(1u << b->token, std::memory_order_release);
    const int final_state = b->state.load(std::memory_order_acquire);
    b->gone[idx].store(1, std::memory_order_release);
    // a slot whose kernel may still be running (failure after the launch) is never handed out again
    if (rc == RING_OK || final_state == 2) free_bit(slot_free, slot);
    if (b->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) free_bit(batch_free, (uint32_t)(b - batches));
    return rc;
}

}  // namespace

bool ring_engaged(const DecodeMode& mode) { return g_ring->engaged(mode); }
int ring_call(const DecodeMode& mode, uint32_t framebits, const unsigned int* symbols, unsigned char* out) {
    return g_ring->call(mode, framebits, symbols, out);
}
int ring_set_window_us(int microseconds) {
    if (microseconds < 0) microseconds = 0;
    if (microseconds > 100000) microseconds = 100000;
    if (g_rstat.on) g_rstat.print_and_reset();
    return g_ring->window_us.exchange(microseconds);
}
int ring_set_min_callers(int n) {
    if (n < 1) n = 1;
    return g_ring->min_callers.exchange(n);
}
int ring_set_depth(int launches_in_flight) { return g_ring->set_depth(launches_in_flight); }
int ring_set_spin_cpus(int cpus) { return g_ring->spin_cpus.exchange(cpus < 0 ? 0 : cpus); }
RingInflight::RingInflight() { g_ring->inflight.fetch_add(1, std::memory_order_relaxed); }
RingInflight::~RingInflight() { g_ring->inflight.fetch_sub(1, std::memory_order_relaxed); }
