// Dev-only: lets pk_device.hpp and pk_table_kernels.hpp compile with g++ as a real 64-LANE wavefront: one OS thread per lane, one wave at
// a time, every cross-lane primitive a rendezvous of the lanes that are still inside the kernel.  What hip_shim.h (one lane: __ballot(p) = p)
// cannot run -- the showdown queue and its prefix sums, the PK_QSYNC hand-offs, two hands per lane, the lone-table paths, parking, the action
// ring -- runs here under ASan / UBSan / TSan (tools/host_sim/sanitize_wave.sh).  Not part of the product.
//
//   * A rendezvous carries its call site (__builtin_FILE / __builtin_LINE).  Lanes that meet at DIFFERENT sites -- a collective placed in
//     divergent control flow -- or a lane that does not turn up within PK_WAVE_SIM_TIMEOUT_MS (default 20 000) are reported with the sites
//     and lane sets, and the program exits with status 3.  It never hangs.
//   * __ballot / __any / readlane / readfirstlane / __shfl_down exchange their values through RELAXED atomics (under TSan; sequentially consistent
//     otherwise): they order nothing, as on the device, where a ballot is no fence for the compiler.  __syncthreads and PK_QSYNC add a
//     release / acquire pair on one atomic word, which TSan understands: an LDS hand-off that lacks its barrier is a reported data race.
//     (Relaxed atomics keep their order here because every read-modify-write is a full barrier on x86-64 and a compiler fence sits between
//     the steps; on another host build without TSan.)
//   * LDS is one heap allocation per wave of exactly sizeof(LDS) bytes, filled with PK_SIM_LDS_GARBAGE before every launch: real LDS is
//     not zeroed, and ASan bounds the object.  The byte reads as a card with rank nibble 13, so that garbage taken for a hand indexes
//     past the evaluator's table.
#pragma once
#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#define PK_WAVE 64
#define PK_WAVE_SIM 1
#define __device__
#define __constant__
#define __global__
#define __forceinline__ inline __attribute__((always_inline))
#define __shared__ static
#define __launch_bounds__(...)
struct uint4 { unsigned x, y, z, w; };
struct dim3_ { unsigned x = 0, y = 0, z = 0; };
inline thread_local dim3_ threadIdx, blockIdx;
static inline int __popc(unsigned x) { return __builtin_popcount(x); }
static inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
static inline int __ffs(unsigned x) { return __builtin_ffs((int)x); }
static inline int __ffsll(long long x) { return __builtin_ffsll(x); }
static inline int __clz(int x) { return x ? __builtin_clz((unsigned)x) : 32; }
static inline unsigned __umulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }
static inline unsigned __umul24(unsigned a, unsigned b) { return (a & 0xffffffu) * (b & 0xffffffu); }
static inline long long __double_as_longlong(double d) { long long v; memcpy(&v, &d, 8); return v; }
static inline void __builtin_amdgcn_s_waitcnt(int) {}
static inline const void *__builtin_amdgcn_kernarg_segment_ptr() { abort(); }   // (the __global__ wrappers are parsed, never run: the driver calls the bodies)
using std::max;
using std::min;

#if defined(__SANITIZE_THREAD__)
#define PK_SIM_MO std::memory_order_relaxed
#else
#define PK_SIM_MO std::memory_order_seq_cst
#endif
#define PK_SIM_LDS_GARBAGE 0x2D

namespace pk_sim {
enum Kind : uint32_t { K_BALLOT = 1, K_READLANE = 2, K_READFIRST = 3, K_SHFL = 4, K_BARRIER = 5, K_DPP = 6 };
inline const char *kind_name(uint32_t k) {
    static const char *n[] = {"?", "__ballot/__any", "readlane", "readfirstlane", "__shfl_down", "barrier (__syncthreads / PK_QSYNC)", "update_dpp"};
    return n[k <= 6 ? k : 0];
}
struct Wave {
    std::atomic<uint64_t> live{0}, pending{0}, arrived[2], val[2][64], hb{0};
    std::atomic<uint32_t> gen{0}, line[64], kind[64], reported{0};
    std::atomic<const char *> file[64];
    void *lds = nullptr;
    size_t lds_bytes = 0;
    int block = 0;
};
inline Wave g_wave;
// wave_sim --ring-stats: what ActionRing::ensure did (PK_RING_COUNT in pk_device.hpp): [0] calls (= loop iterations of rollout_body), [1] Philox
// passes, [2] lanes filled by them; counted by one lane per wave ([0], [1]) or by every filling lane ([2])
inline std::atomic<uint64_t> ring_count[3];
#define PK_RING_COUNT(k, n) pk_sim::ring_count[k].fetch_add((n), std::memory_order_relaxed)
inline thread_local int t_lane = -1;
inline void cfence() { std::atomic_signal_fence(std::memory_order_seq_cst); }
inline int timeout_ms() {
    static const int ms = [] { const char *e = getenv("PK_WAVE_SIM_TIMEOUT_MS"); return e && atoi(e) > 0 ? atoi(e) : 20000; }();
    return ms;
}
inline void print_set(uint64_t m) {
    if (!m) { fprintf(stderr, "(none)"); return; }
    for (int l = 0; l < 64; ++l)
        if ((m >> l) & 1) {
            int e = l;
            while (e + 1 < 64 && ((m >> (e + 1)) & 1)) ++e;
            if (e > l) fprintf(stderr, "%d-%d ", l, e); else fprintf(stderr, "%d ", l);
            l = e;
        }
}
// the sites the lanes of `am` wait at, grouped; then out
[[noreturn]] inline void report(const char *what, uint64_t am, uint64_t missing) {
    Wave &w = g_wave;
    if (w.reported.exchange(1)) for (;;) pause();   // one report; the reporting lane ends the process
    fprintf(stderr, "wave_sim: %s (workgroup %d)\n", what, w.block);
    uint64_t todo = am;
    while (todo) {
        const int l0 = __builtin_ctzll(todo);
        uint64_t same = 0;
        for (int l = l0; l < 64; ++l)
            if (((todo >> l) & 1) && w.line[l].load() == w.line[l0].load() && w.file[l].load() == w.file[l0].load() && w.kind[l].load() == w.kind[l0].load()) same |= 1ull << l;
        const char *f = w.file[l0].load(), *s = f ? strrchr(f, '/') : nullptr;
        fprintf(stderr, "  %s at %s:%u: lanes ", kind_name(w.kind[l0].load()), s ? s + 1 : (f ? f : "?"), w.line[l0].load());
        print_set(same);
        fprintf(stderr, "\n");
        todo &= ~same;
    }
    if (missing) { fprintf(stderr, "  inside the kernel, at no rendezvous: lanes "); print_set(missing); fprintf(stderr, "\n"); }
    fflush(stderr);
    _exit(3);
}
// every live lane has arrived (or left): same site everywhere?  Then open the next generation.
inline void complete(uint32_t g) {
    Wave &w = g_wave;
    const int par = g & 1;
    const uint64_t am = w.arrived[par].load(PK_SIM_MO);
    const int l0 = __builtin_ctzll(am);
    for (int l = l0 + 1; l < 64; ++l)
        if (((am >> l) & 1) && (w.line[l].load(PK_SIM_MO) != w.line[l0].load(PK_SIM_MO) || w.file[l].load(PK_SIM_MO) != w.file[l0].load(PK_SIM_MO) ||
                                w.kind[l].load(PK_SIM_MO) != w.kind[l0].load(PK_SIM_MO)))
            report("lanes of one wave meet at DIFFERENT collectives (a collective in divergent control flow)", am, 0);
    w.arrived[par ^ 1].store(0, PK_SIM_MO);
    w.pending.store(w.live.load(PK_SIM_MO), PK_SIM_MO);
    cfence();
    w.gen.store(g + 1, PK_SIM_MO);
    syscall(SYS_futex, reinterpret_cast<uint32_t *>(&w.gen), FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
}
inline void wait_gen(uint32_t g) {
    Wave &w = g_wave;
    for (int i = 0; i < 64; ++i) { if (w.gen.load(PK_SIM_MO) != g) return; __builtin_ia32_pause(); }
    const auto t0 = std::chrono::steady_clock::now();
    while (w.gen.load(PK_SIM_MO) == g) {
        struct timespec ts = {0, 200 * 1000 * 1000};
        syscall(SYS_futex, reinterpret_cast<uint32_t *>(&w.gen), FUTEX_WAIT_PRIVATE, g, &ts, nullptr, 0);
        if (w.gen.load(PK_SIM_MO) != g) return;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(timeout_ms()))
            report("a lane is missing at a collective (waited PK_WAVE_SIM_TIMEOUT_MS)", w.arrived[g & 1].load(), w.pending.load());
    }
}
// One rendezvous of the lanes still inside the kernel; returns the parity of its generation (whose val[] / arrived[] hold the exchange).
inline int meet(uint32_t kind, uint64_t v, const char *file, int line) {
    Wave &w = g_wave;
    const int lane = t_lane;
    const uint64_t bit = 1ull << lane;
    const uint32_t g = w.gen.load(PK_SIM_MO);
    const int par = g & 1;
    w.val[par][lane].store(v, PK_SIM_MO);
    w.line[lane].store((uint32_t)line, PK_SIM_MO); w.file[lane].store(file, PK_SIM_MO); w.kind[lane].store(kind, PK_SIM_MO);
    if (kind == K_BARRIER) w.hb.fetch_add(1, std::memory_order_release);
    cfence();
    w.arrived[par].fetch_or(bit, PK_SIM_MO);
    cfence();
    const uint64_t prev = w.pending.fetch_and(~bit, PK_SIM_MO);
    cfence();
    if ((prev & ~bit) == 0) complete(g); else wait_gen(g);
    cfence();
    if (kind == K_BARRIER) (void)w.hb.load(std::memory_order_acquire);
    return par;
}
// a lane returns from the kernel: it drops out of every later rendezvous (and may be the one the others were waiting for)
inline void leave() {
    Wave &w = g_wave;
    const uint64_t bit = 1ull << t_lane;
    const uint32_t g = w.gen.load(PK_SIM_MO);
    w.live.fetch_and(~bit, PK_SIM_MO);
    cfence();
    const uint64_t prev = w.pending.fetch_and(~bit, PK_SIM_MO);
    cfence();
    if ((prev & bit) && (prev & ~bit) == 0 && w.arrived[g & 1].load(PK_SIM_MO) != 0) complete(g);
}
inline unsigned long long ballot(int p, const char *file, int line) {
    const int par = meet(K_BALLOT, p ? 1 : 0, file, line);
    const uint64_t am = g_wave.arrived[par].load(PK_SIM_MO);
    unsigned long long r = 0;
    for (int l = 0; l < 64; ++l) if (((am >> l) & 1) && g_wave.val[par][l].load(PK_SIM_MO)) r |= 1ull << l;
    return r;
}
// The wave's LDS object (the driver sized the allocation with the same type)
inline void *lds_object(size_t bytes) {
    if (bytes != g_wave.lds_bytes) { fprintf(stderr, "wave_sim: the kernel's LDS object has %zu bytes, the launch allocated %zu\n", bytes, g_wave.lds_bytes); _exit(3); }
    return g_wave.lds;
}
[[noreturn]] inline void index_fail(const char *what, unsigned long long i, unsigned long long n, const char *file, int line) {
    const char *s = strrchr(file, '/');
    fprintf(stderr, "wave_sim: index out of range: %s: %llu, limit %llu, at %s:%d (workgroup %d, lane %d)\n", what, i, n, s ? s + 1 : file, line, g_wave.block, t_lane);
    fflush(stderr);
    abort();
}
// Runs body() as `grid` one-wave workgroups, one after the other, 64 threads each.
template <typename F>
inline void launch(int grid, size_t lds_bytes, F &&body) {
    Wave &w = g_wave;
    for (int b = 0; b < grid; ++b) {
        w.lds = malloc(lds_bytes ? lds_bytes : 1); w.lds_bytes = lds_bytes; w.block = b;
        memset(w.lds, PK_SIM_LDS_GARBAGE, lds_bytes);
        w.live.store(~0ull); w.pending.store(~0ull); w.arrived[0].store(0); w.arrived[1].store(0); w.gen.store(0);
        std::vector<std::thread> th;
        th.reserve(64);
        for (int l = 0; l < 64; ++l)
            th.emplace_back([&body, b, l] {
                threadIdx.x = (unsigned)l; blockIdx.x = (unsigned)b; t_lane = l;
                body();
                leave();
            });
        for (auto &t : th) t.join();
        free(w.lds); w.lds = nullptr;
    }
}
}  // namespace pk_sim

#define PK_SIM_SITE const char *file = __builtin_FILE(), int line = __builtin_LINE()
static inline unsigned long long __ballot(int p, PK_SIM_SITE) { return pk_sim::ballot(p, file, line); }
static inline int __any(int p, PK_SIM_SITE) { return pk_sim::ballot(p, file, line) != 0; }
static inline void __syncthreads(PK_SIM_SITE) { pk_sim::meet(pk_sim::K_BARRIER, 0, file, line); }
static inline int __builtin_amdgcn_readlane(int v, int lane, PK_SIM_SITE) {   // `lane` is wave-uniform and active
    const int par = pk_sim::meet(pk_sim::K_READLANE, (uint32_t)v | ((uint64_t)(uint32_t)lane << 32), file, line);
    const uint64_t am = pk_sim::g_wave.arrived[par].load(PK_SIM_MO);
    if (lane < 0 || lane > 63 || !((am >> lane) & 1)) pk_sim::report("readlane of a lane that is not active", am, 0);
    return (int)(uint32_t)pk_sim::g_wave.val[par][lane].load(PK_SIM_MO);
}
static inline int __builtin_amdgcn_readfirstlane(int v, PK_SIM_SITE) {
    const int par = pk_sim::meet(pk_sim::K_READFIRST, (uint32_t)v, file, line);
    return (int)(uint32_t)pk_sim::g_wave.val[par][__builtin_ctzll(pk_sim::g_wave.arrived[par].load(PK_SIM_MO))].load(PK_SIM_MO);
}
static inline unsigned __shfl_down(unsigned v, int off, int width, PK_SIM_SITE) {   // an inactive or out-of-range source: the lane's own value
    (void)width;
    const int par = pk_sim::meet(pk_sim::K_SHFL, v, file, line), src = pk_sim::t_lane + off;
    const uint64_t am = pk_sim::g_wave.arrived[par].load(PK_SIM_MO);
    return (src < 64 && ((am >> src) & 1)) ? (unsigned)pk_sim::g_wave.val[par][src].load(PK_SIM_MO) : v;
}
// v_mov_b32_dpp for the controls wave_excl_scan (pk_device.hpp) uses: row_shr:1..15 (0x111..0x11f: the lane n below in the same row of 16),
// row_bcast:15 (0x142: lane 15 of the row below) and row_bcast:31 (0x143: lane 31, for rows 2 and 3).  A lane whose row or bank the masks
// leave out keeps `old`; so does one whose source is out of range or not active, unless bound_ctrl asks for 0.  Any other control aborts.
static inline int __builtin_amdgcn_update_dpp(int old, int src, int ctrl, int row_mask, int bank_mask, bool bound_ctrl, PK_SIM_SITE) {
    const int par = pk_sim::meet(pk_sim::K_DPP, (uint32_t)src, file, line), l = pk_sim::t_lane;
    const uint64_t am = pk_sim::g_wave.arrived[par].load(PK_SIM_MO);
    int from = -1;
    bool in_range = true;
    if (ctrl >= 0x111 && ctrl <= 0x11f) { from = l - (ctrl - 0x110); in_range = (l & 15) >= ctrl - 0x110; }
    else if (ctrl == 0x142) { from = (l & ~15) - 1; in_range = l >= 16; }
    else if (ctrl == 0x143) { from = 31; in_range = l >= 32; }
    else { fprintf(stderr, "wave_sim: update_dpp control 0x%x is not implemented\n", ctrl); abort(); }
    if (!((row_mask >> (l >> 4)) & 1) || !((bank_mask >> ((l >> 2) & 3)) & 1)) return old;
    if (!in_range || !((am >> from) & 1)) return bound_ctrl ? 0 : old;
    return (int)(uint32_t)pk_sim::g_wave.val[par][from].load(PK_SIM_MO);
}
// lanes below this one among the mask's bits (v_mbcnt_lo / _hi_u32_b32)
static inline unsigned __builtin_amdgcn_mbcnt_lo(unsigned mask, unsigned v) {
    const int l = pk_sim::t_lane;
    return v + (unsigned)__builtin_popcount(l >= 32 ? mask : (mask & ((1u << l) - 1u)));
}
static inline unsigned __builtin_amdgcn_mbcnt_hi(unsigned mask, unsigned v) {
    const int l = pk_sim::t_lane;
    return v + (unsigned)__builtin_popcount(l <= 32 ? 0u : (mask & ((1u << (l - 32)) - 1u)));
}
