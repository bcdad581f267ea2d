// Dev-only: lets the equity kernels (pokerl_amd/csrc/pk_equity*.hip) compile with g++ and run as REAL MULTI-WAVE WORKGROUPS -- 8 waves x 64
// lanes, the 256-thread preparation kernels as 4 x 64 -- on the CPU, under ASan / UBSan / TSan (tools/host_sim/sanitize_equity.sh).  The
// sibling of wave_shim.h (one 64-lane wave per workgroup, the table kernels); the kernel bodies are the unmodified ones.  Not part of the product.
//
//   * A LANE IS A FIBRE (ucontext), all of a workgroup's on one OS thread, run round robin by the launch loop until each waits at a
//     rendezvous or has returned.  A barrier of 512 lanes is 512 context switches (about 0.1 ms; 512 OS threads: 3 ms, 23 ms under TSan), and the
//     schedule is the same in every run.  TSan is told of every fibre (__tsan_create_fiber / __tsan_switch_to_fiber with the no-sync flag): each
//     lane has its own clock, and a switch orders nothing.
//   * Per-wave collectives -- __shfl / __shfl_up / __shfl_down / __shfl_xor (32 and 64 bits), __ballot / __any, readlane / readfirstlane,
//     __builtin_amdgcn_wave_barrier -- are a rendezvous of that wave's lanes that are still inside the kernel; __syncthreads is one of all the
//     workgroup's.  A rendezvous carries its call site.  Lanes that meet at DIFFERENT sites, a wave whose lanes are split between a wave
//     collective and __syncthreads, a shuffle whose source lane has left, a workgroup in which nothing can run any more (a lane that never
//     turns up): each is reported with the sites and lane sets, and the program exits with status 3.  It never hangs.
//   * What TSan sees.  __syncthreads is a release / acquire pair on the workgroup's word: the ONLY edge between waves, so a hand-off from one
//     wave to another that lacks its barrier is a reported race.  A wave collective is a release / acquire pair on that WAVE's word: a wave is one
//     instruction stream whose LDS operations execute in issue order (pk_device.hpp, "The showdown queue's synchronisation points"), so what
//     a lane did before a cross-lane instruction is done for every lane of the wave after it; two lanes of one wave that touch one word with
//     no collective between them are still a reported race.  __builtin_amdgcn_fence is a compiler fence and orders nothing more.
//     (wave_shim.h keeps its ballots relaxed to pin the table kernels' PK_QSYNC; k_equity's per-wave pools are handed on through
//     shuffle + fence, which is exactly the issue-order argument.)
//   * atomicAdd (uint32_t, unsigned long long; LDS and global) is a relaxed atomic read-modify-write.
//   * threadIdx / blockIdx / blockDim / gridDim exist (.x); workgroups of a grid run one after the other: no equity kernel waits for another.
//   * LDS.  `__shared__` is `static`: the kernels' function-local arrays become statics that ASan bounds with redzones.  The launch finds them in
//     the program's own symbol table (lds_find: the objects local to the functions named) and fills every one with PK_SIM_LDS_GARBAGE before
//     EVERY workgroup: real LDS is not zeroed, and holds what the workgroup before left.  The byte is wave_shim.h's, for its reason: it reads as
//     a card with rank nibble 13, so that garbage taken for a hand indexes past the evaluator's table.  (Link without -s.)
//   * PK_IDX is active (pk_device.hpp under PK_WAVE_SIM) and aborts with the array's name and the site.
#pragma once
#include <elf.h>
#include <fcntl.h>
#include <link.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <ucontext.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#if defined(__SANITIZE_THREAD__)
extern "C" {
void *__tsan_get_current_fiber(void);
void *__tsan_create_fiber(unsigned flags);
void __tsan_destroy_fiber(void *fiber);
void __tsan_switch_to_fiber(void *fiber, unsigned flags);
}
#endif
#if defined(__SANITIZE_ADDRESS__)
extern "C" {
void __sanitizer_start_switch_fiber(void **fake_stack_save, const void *bottom, size_t size);
void __sanitizer_finish_switch_fiber(void *fake_stack_save, const void **bottom_old, size_t *size_old);
}
#endif

#define PK_WAVE 64
#define PK_WAVE_SIM 1
#define PK_WG_SIM 1
#define __device__
#define __host__
#define __constant__
#define __global__
#define __forceinline__ inline __attribute__((always_inline))
#define __shared__ static
#define __launch_bounds__(...)
struct uint4 { unsigned x, y, z, w; };
struct uint2 { unsigned x, y; };
static inline uint2 make_uint2(unsigned x, unsigned y) { return uint2{x, y}; }
static inline int __popc(unsigned x) { return __builtin_popcount(x); }
static inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
static inline int __ffs(unsigned x) { return __builtin_ffs((int)x); }
static inline int __ffsll(long long x) { return __builtin_ffsll(x); }
static inline int __clz(int x) { return x ? __builtin_clz((unsigned)x) : 32; }
static inline unsigned __umulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }
static inline unsigned __umul24(unsigned a, unsigned b) { return (a & 0xffffffu) * (b & 0xffffffu); }
static inline long long __double_as_longlong(double d) { long long v; memcpy(&v, &d, 8); return v; }
static inline void __builtin_amdgcn_s_waitcnt(int) {}
using std::max;
using std::min;
// the host launch functions at the bottom of the .hip files are parsed, never run: the driver calls the kernels
typedef int hipError_t;
typedef void *hipStream_t;
enum { hipSuccess = 0, hipErrorInvalidValue = 1 };
struct dim3 { unsigned x, y, z; explicit dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {} };
static inline hipError_t hipGetLastError() { return hipSuccess; }
static inline hipError_t hipMemsetAsync(void *, int, size_t, hipStream_t) { abort(); }
#define hipLaunchKernelGGL(...) abort()

#define PK_SIM_MO std::memory_order_relaxed
#define PK_SIM_LDS_GARBAGE 0x2D

namespace pk_sim {
enum Kind : uint32_t { K_NONE = 0, K_BALLOT, K_READLANE, K_READFIRST, K_SHFL, K_WAVE_BARRIER, K_SYNCTHREADS };
inline const char *kind_name(uint32_t k) {
    static const char *n[] = {"?", "__ballot/__any", "readlane", "readfirstlane", "__shfl*", "wave_barrier", "__syncthreads"};
    return n[k <= 6 ? k : 0];
}
enum LaneState : uint32_t { L_READY = 0, L_WAIT_WAVE, L_WAIT_WG, L_DONE };
constexpr int MAX_LANES = 1024, MAX_WAVES = MAX_LANES / 64;
constexpr size_t STACK_BYTES = 128 * 1024;   // (ASan clears a stack's whole shadow at every switch to it: a large one costs an mmap each time)

// Everything the launch loop and the lanes share is a relaxed atomic: the shim's own traffic orders nothing for TSan.
struct Lane {
    ucontext_t ctx;
    void *stack = nullptr, *tsan = nullptr;
    std::atomic<uint32_t> state{L_DONE}, kind{0}, line{0};
    std::atomic<const char *> file{nullptr};
    std::atomic<uint64_t> val{0};
};
struct Group {
    Lane lane[MAX_LANES];
    ucontext_t main_ctx;
    std::atomic<void *> main_tsan{nullptr};
    std::atomic<int> cur{-1}, nlanes{0}, block{0};
    std::atomic<unsigned> grid{1}, bdim{64};
    std::atomic<uint64_t> xval[MAX_WAVES][64], xmask[MAX_WAVES];
    // the words TSan's happens-before edges hang on.  Two per wave and per workgroup, used in turn: a lane that runs on to its NEXT rendezvous
    // releases on the other word, so a lane that is resumed later acquires what was released AT the rendezvous it waited at and nothing newer
    // (with one word the lanes resumed late would inherit, falsely, all that the first ones did since).
    std::atomic<uint64_t> hb_wave[MAX_WAVES][2], hb_wg[2], hb_launch{0};
    std::atomic<uint32_t> gen_wave[MAX_WAVES], gen_wg{0};                 // rendezvous completed so far
    std::atomic<void (*)(void *)> body{nullptr};
    std::atomic<void *> body_arg{nullptr};
    unsigned long long rendezvous = 0, barriers = 0;
};
inline Group g;
struct LdsObject { char *p; size_t n; std::string name; };
inline std::vector<LdsObject> g_lds;

inline int cur_lane() { return g.cur.load(PK_SIM_MO); }
inline void cfence() { std::atomic_signal_fence(std::memory_order_seq_cst); }

inline void print_set(const std::vector<int> &v) {
    for (size_t i = 0; i < v.size(); ++i) {
        size_t e = i;
        while (e + 1 < v.size() && v[e + 1] == v[e] + 1) ++e;
        if (e > i) fprintf(stderr, "%d-%d ", v[i], v[e]); else fprintf(stderr, "%d ", v[i]);
        i = e;
    }
}
// where every lane that is still inside the kernel waits, grouped by site; then out
[[noreturn]] inline void report(const char *what) {
    const int n = g.nlanes.load(PK_SIM_MO);
    fprintf(stderr, "wg_sim: %s (workgroup %d of %u, %d lanes)\n", what, g.block.load(PK_SIM_MO), g.grid.load(PK_SIM_MO), n);
    std::vector<char> seen(n, 0);
    for (int l0 = 0; l0 < n; ++l0) {
        const uint32_t st = g.lane[l0].state.load(PK_SIM_MO);
        if (seen[l0] || st == L_DONE || st == L_READY) continue;
        std::vector<int> same;
        for (int l = l0; l < n; ++l) {
            const uint32_t s2 = g.lane[l].state.load(PK_SIM_MO);
            if (!seen[l] && s2 != L_DONE && s2 != L_READY && g.lane[l].line.load(PK_SIM_MO) == g.lane[l0].line.load(PK_SIM_MO) &&
                g.lane[l].file.load(PK_SIM_MO) == g.lane[l0].file.load(PK_SIM_MO) && g.lane[l].kind.load(PK_SIM_MO) == g.lane[l0].kind.load(PK_SIM_MO)) { same.push_back(l); seen[l] = 1; }
        }
        const char *f = g.lane[l0].file.load(PK_SIM_MO), *s = f ? strrchr(f, '/') : nullptr;
        fprintf(stderr, "  %s at %s:%u: lanes ", kind_name(g.lane[l0].kind.load(PK_SIM_MO)), s ? s + 1 : (f ? f : "?"), g.lane[l0].line.load(PK_SIM_MO));
        print_set(same);
        fprintf(stderr, "\n");
    }
    std::vector<int> gone;
    for (int l = 0; l < n; ++l) if (g.lane[l].state.load(PK_SIM_MO) == L_DONE) gone.push_back(l);
    if (!gone.empty()) { fprintf(stderr, "  have left the kernel: lanes "); print_set(gone); fprintf(stderr, "\n"); }
    fflush(stderr);
    _exit(3);
}
[[noreturn]] inline void index_fail(const char *what, unsigned long long i, unsigned long long n, const char *file, int line) {
    const char *s = strrchr(file, '/');
    fprintf(stderr, "wg_sim: index out of range: %s: %llu, limit %llu, at %s:%d (workgroup %d, lane %d)\n", what, i, n, s ? s + 1 : file, line, g.block.load(PK_SIM_MO), cur_lane());
    fflush(stderr);
    abort();
}
inline void *lds_object(size_t) { fprintf(stderr, "wg_sim: PK_SHARED_OBJECT is the table kernels' (wave_shim.h)\n"); abort(); }

// ---- context switches, with the sanitizers told
inline void switch_ctx(ucontext_t *from, ucontext_t *to, [[maybe_unused]] void *to_tsan, [[maybe_unused]] const void *to_stack, [[maybe_unused]] size_t to_bytes) {
#if defined(__SANITIZE_ADDRESS__)
    void *fake = nullptr;
    __sanitizer_start_switch_fiber(&fake, to_stack, to_bytes);
#endif
#if defined(__SANITIZE_THREAD__)
    __tsan_switch_to_fiber(to_tsan, 1u /* no synchronisation */);
#endif
    swapcontext(from, to);
#if defined(__SANITIZE_ADDRESS__)
    __sanitizer_finish_switch_fiber(fake, nullptr, nullptr);
#endif
}
inline const void *g_main_stack = nullptr;
inline size_t g_main_stack_bytes = 0;
// a lane gives way to the launch loop
inline void yield_lane(int l) { switch_ctx(&g.lane[l].ctx, &g.main_ctx, g.main_tsan.load(PK_SIM_MO), g_main_stack, g_main_stack_bytes); }

// One rendezvous: the lane records where it waits and gives way; the launch loop wakes it once its wave (or workgroup) is complete.
inline int meet(uint32_t kind, uint64_t v, const char *file, int line) {
    const int l = cur_lane(), w = l >> 6;
    Lane &me = g.lane[l];
    me.val.store(v, PK_SIM_MO); me.kind.store(kind, PK_SIM_MO); me.line.store((uint32_t)line, PK_SIM_MO); me.file.store(file, PK_SIM_MO);
    std::atomic<uint64_t> &hb = kind == K_SYNCTHREADS ? g.hb_wg[g.gen_wg.load(PK_SIM_MO) & 1u] : g.hb_wave[w][g.gen_wave[w].load(PK_SIM_MO) & 1u];
    hb.fetch_add(1, std::memory_order_release);
    cfence();
    me.state.store(kind == K_SYNCTHREADS ? L_WAIT_WG : L_WAIT_WAVE, PK_SIM_MO);
    yield_lane(l);
    cfence();
    (void)hb.load(std::memory_order_acquire);
    return l;
}
inline uint64_t wave_mask(int l) { return g.xmask[l >> 6].load(PK_SIM_MO); }
inline uint64_t wave_val(int l, int src) { return g.xval[l >> 6][src].load(PK_SIM_MO); }
[[noreturn]] inline void lane_fail(const char *what, int src, const char *file, int line) {
    const char *s = strrchr(file, '/');
    fprintf(stderr, "wg_sim: %s: source lane %d, at %s:%d (workgroup %d, lane %d)\n", what, src, s ? s + 1 : file, line, g.block.load(PK_SIM_MO), cur_lane());
    fflush(stderr);
    _exit(3);
}

inline void trampoline() {
#if defined(__SANITIZE_ADDRESS__)
    __sanitizer_finish_switch_fiber(nullptr, &g_main_stack, &g_main_stack_bytes);
#endif
    const int l = cur_lane();
    (void)g.hb_launch.load(std::memory_order_acquire);          // what the host wrote before the launch
    g.body.load(PK_SIM_MO)(g.body_arg.load(PK_SIM_MO));
    g.hb_launch.fetch_add(1, std::memory_order_release);         // ... and what it reads after it
    g.lane[l].state.store(L_DONE, PK_SIM_MO);
    yield_lane(l);
    abort();                                                     // (a lane that has left is never resumed)
}

// ---- the kernels' function-local __shared__ arrays, out of the program's own symbol table: every OBJECT symbol "_ZZ<function>E<name>" whose
// function's mangled name holds one of `fragments` (e.g. "5k_rvr").  Returns the bytes found.
inline size_t lds_find(const std::vector<std::string> &fragments) {
    g_lds.clear();
    uintptr_t bias = 0;
    dl_iterate_phdr([](struct dl_phdr_info *info, size_t, void *p) { *(uintptr_t *)p = info->dlpi_addr; return 1; }, &bias);   // (the first entry is the program)
    const int fd = open("/proc/self/exe", O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0) { perror("wg_sim: /proc/self/exe"); _exit(2); }
    const char *img = (const char *)mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (img == MAP_FAILED) { perror("wg_sim: mmap"); _exit(2); }
    const Elf64_Ehdr *eh = (const Elf64_Ehdr *)img;
    const Elf64_Shdr *sh = (const Elf64_Shdr *)(img + eh->e_shoff);
    size_t total = 0;
    for (int i = 0; i < eh->e_shnum; ++i) {
        if (sh[i].sh_type != SHT_SYMTAB) continue;
        const Elf64_Sym *sym = (const Elf64_Sym *)(img + sh[i].sh_offset);
        const char *str = img + sh[sh[i].sh_link].sh_offset;
        for (size_t k = 0; k < sh[i].sh_size / sizeof(Elf64_Sym); ++k) {
            if (ELF64_ST_TYPE(sym[k].st_info) != STT_OBJECT || sym[k].st_size == 0 || sym[k].st_shndx == SHN_UNDEF) continue;
            const char *nm = str + sym[k].st_name;
            if (strncmp(nm, "_ZZ", 3) != 0) continue;
            if (!(sh[sym[k].st_shndx].sh_flags & SHF_WRITE)) continue;
            bool hit = false;
            for (const std::string &f : fragments) if (strstr(nm, f.c_str())) hit = true;
            if (!hit) continue;
            g_lds.push_back(LdsObject{(char *)(bias + sym[k].st_value), (size_t)sym[k].st_size, nm});
            total += (size_t)sym[k].st_size;
        }
    }
    munmap((void *)img, (size_t)sb.st_size);
    close(fd);
    return total;
}
inline void lds_garbage() { for (const LdsObject &o : g_lds) memset(o.p, PK_SIM_LDS_GARBAGE, o.n); }

// Runs body() as `grid` workgroups of `block` lanes (a multiple of 64), one after the other.
template <typename F>
inline void launch(unsigned grid, unsigned block, F &&body) {
    if (block == 0 || block > MAX_LANES || (block & 63u)) { fprintf(stderr, "wg_sim: a workgroup of %u lanes\n", block); _exit(2); }
    if (g_lds.empty()) { fprintf(stderr, "wg_sim: no LDS object registered (lds_find) -- garbage LDS is part of every launch\n"); _exit(2); }
    const int n = (int)block, nw = n / 64;
    g.body.store([](void *p) { (*static_cast<std::remove_reference_t<F> *>(p))(); }, PK_SIM_MO);
    g.body_arg.store((void *)&body, PK_SIM_MO);
    g.grid.store(grid, PK_SIM_MO); g.bdim.store(block, PK_SIM_MO); g.nlanes.store(n, PK_SIM_MO);
#if defined(__SANITIZE_THREAD__)
    g.main_tsan.store(__tsan_get_current_fiber(), PK_SIM_MO);
#endif
    for (unsigned b = 0; b < grid; ++b) {
        g.block.store((int)b, PK_SIM_MO);
        lds_garbage();
        for (int l = 0; l < n; ++l) {
            Lane &L = g.lane[l];
            if (!L.stack) {
                L.stack = mmap(nullptr, STACK_BYTES, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
                if (L.stack == MAP_FAILED) { perror("wg_sim: a lane's stack"); _exit(2); }
                mprotect(L.stack, 4096, PROT_NONE);                            // (a stack that overflows faults at once)
            }
            getcontext(&L.ctx);
            L.ctx.uc_stack.ss_sp = L.stack; L.ctx.uc_stack.ss_size = STACK_BYTES; L.ctx.uc_link = nullptr;
            makecontext(&L.ctx, trampoline, 0);
#if defined(__SANITIZE_THREAD__)
            L.tsan = __tsan_create_fiber(0);
#endif
            L.state.store(L_READY, PK_SIM_MO);
        }
        g.hb_launch.fetch_add(1, std::memory_order_release);
        int live = n;
        while (live) {
            bool ran = false;
            for (int l = 0; l < n; ++l) {
                Lane &L = g.lane[l];
                if (L.state.load(PK_SIM_MO) != L_READY) continue;
                g.cur.store(l, PK_SIM_MO);
                switch_ctx(&g.main_ctx, &L.ctx, L.tsan, L.stack, STACK_BYTES);
                g.cur.store(-1, PK_SIM_MO);
                ran = true;
                if (L.state.load(PK_SIM_MO) == L_DONE) --live;
            }
            if (!live) break;
            // every lane now waits or has left.  Waves first: all of a wave's lanes at ONE wave collective -> the exchange is published, they go on.
            bool woke = false;
            int at_wg = 0;
            for (int w = 0; w < nw; ++w) {
                uint64_t wave_m = 0, wg_m = 0;
                for (int i = 0; i < 64; ++i) {
                    const uint32_t st = g.lane[w * 64 + i].state.load(PK_SIM_MO);
                    if (st == L_WAIT_WAVE) wave_m |= 1ull << i;
                    if (st == L_WAIT_WG) wg_m |= 1ull << i;
                }
                at_wg += __builtin_popcountll(wg_m);
                if (!wave_m) continue;
                if (wg_m) report("one wave's lanes are split between a wave collective and __syncthreads (a collective in divergent control flow)");
                const Lane &L0 = g.lane[w * 64 + __builtin_ctzll(wave_m)];
                for (int i = 0; i < 64; ++i)
                    if ((wave_m >> i) & 1) {
                        const Lane &L = g.lane[w * 64 + i];
                        if (L.line.load(PK_SIM_MO) != L0.line.load(PK_SIM_MO) || L.file.load(PK_SIM_MO) != L0.file.load(PK_SIM_MO) || L.kind.load(PK_SIM_MO) != L0.kind.load(PK_SIM_MO))
                            report("lanes of one wave meet at DIFFERENT collectives (a collective in divergent control flow)");
                        g.xval[w][i].store(L.val.load(PK_SIM_MO), PK_SIM_MO);
                    }
                g.xmask[w].store(wave_m, PK_SIM_MO);
                for (int i = 0; i < 64; ++i) if ((wave_m >> i) & 1) g.lane[w * 64 + i].state.store(L_READY, PK_SIM_MO);
                g.gen_wave[w].fetch_add(1, PK_SIM_MO);
                woke = true;
                ++g.rendezvous;
            }
            if (woke) continue;
            // no wave can go on: then every lane still inside waits at __syncthreads -- at one site
            if (at_wg != live) report("nothing can run any more: a lane never turns up");
            int l0 = -1;
            for (int l = 0; l < n; ++l) {
                Lane &L = g.lane[l];
                if (L.state.load(PK_SIM_MO) != L_WAIT_WG) continue;
                if (l0 < 0) l0 = l;
                if (L.line.load(PK_SIM_MO) != g.lane[l0].line.load(PK_SIM_MO) || L.file.load(PK_SIM_MO) != g.lane[l0].file.load(PK_SIM_MO))
                    report("lanes of one workgroup meet at DIFFERENT __syncthreads (a barrier in divergent control flow)");
            }
            for (int l = 0; l < n; ++l) if (g.lane[l].state.load(PK_SIM_MO) == L_WAIT_WG) g.lane[l].state.store(L_READY, PK_SIM_MO);
            g.gen_wg.fetch_add(1, PK_SIM_MO);
            ++g.barriers;
            (void)ran;
        }
        (void)g.hb_launch.load(std::memory_order_acquire);
#if defined(__SANITIZE_THREAD__)
        for (int l = 0; l < n; ++l) { __tsan_destroy_fiber(g.lane[l].tsan); g.lane[l].tsan = nullptr; }
#endif
    }
}

// threadIdx.x and its kin: read off the lane that is running
struct TidX { operator unsigned() const { return (unsigned)cur_lane(); } };
struct BidX { operator unsigned() const { return (unsigned)g.block.load(PK_SIM_MO); } };
struct BdimX { operator unsigned() const { return g.bdim.load(PK_SIM_MO); } };
struct GdimX { operator unsigned() const { return g.grid.load(PK_SIM_MO); } };
template <typename X> struct Dim { X x; };
}  // namespace pk_sim

inline pk_sim::Dim<pk_sim::TidX> threadIdx;
inline pk_sim::Dim<pk_sim::BidX> blockIdx;
inline pk_sim::Dim<pk_sim::BdimX> blockDim;
inline pk_sim::Dim<pk_sim::GdimX> gridDim;

#define PK_SIM_SITE const char *file = __builtin_FILE(), int line = __builtin_LINE()
static inline void __syncthreads(PK_SIM_SITE) { pk_sim::meet(pk_sim::K_SYNCTHREADS, 0, file, line); }
static inline void __builtin_amdgcn_wave_barrier(PK_SIM_SITE) { pk_sim::meet(pk_sim::K_WAVE_BARRIER, 0, file, line); }
static inline void __builtin_amdgcn_fence(int, const char *) { pk_sim::cfence(); }
static inline unsigned long long __ballot(int p, PK_SIM_SITE) {
    const int l = pk_sim::meet(pk_sim::K_BALLOT, p ? 1 : 0, file, line);
    const uint64_t am = pk_sim::wave_mask(l);
    unsigned long long r = 0;
    for (int i = 0; i < 64; ++i) if (((am >> i) & 1) && pk_sim::wave_val(l, i)) r |= 1ull << i;
    return r;
}
static inline int __any(int p, PK_SIM_SITE) { return __ballot(p, file, line) != 0; }
static inline int __builtin_amdgcn_readlane(int v, int lane, PK_SIM_SITE) {   // `lane` is wave-uniform and active
    const int l = pk_sim::meet(pk_sim::K_READLANE, (uint32_t)v, file, line);
    if (lane < 0 || lane > 63 || !((pk_sim::wave_mask(l) >> lane) & 1)) pk_sim::lane_fail("readlane of a lane that is not active", lane, file, line);
    return (int)(uint32_t)pk_sim::wave_val(l, lane);
}
static inline int __builtin_amdgcn_readfirstlane(int v, PK_SIM_SITE) {
    const int l = pk_sim::meet(pk_sim::K_READFIRST, (uint32_t)v, file, line);
    return (int)(uint32_t)pk_sim::wave_val(l, __builtin_ctzll(pk_sim::wave_mask(l)));
}
namespace pk_sim {
// One shuffle: every lane of the wave gives v; the lane takes lane `src`'s (its own where src is outside the wave, as the device does).  A
// source lane that has left the kernel holds nothing: reported.
template <typename T>
inline T shfl(T v, int src, const char *file, int line) {
    static_assert(std::is_trivially_copyable_v<T> && (sizeof(T) == 4 || sizeof(T) == 8), "32- and 64-bit shuffles");
    uint64_t bits = 0;
    memcpy(&bits, &v, sizeof(T));
    const int l = meet(K_SHFL, bits, file, line);
    if (src < 0 || src > 63) return v;
    if (!((wave_mask(l) >> src) & 1)) lane_fail("shuffle from a lane that is not active", src, file, line);
    bits = wave_val(l, src);
    T r;
    memcpy(&r, &bits, sizeof(T));
    return r;
}
}  // namespace pk_sim
template <typename T> static inline T __shfl(T v, int src, int width = 64, PK_SIM_SITE) { (void)width; return pk_sim::shfl(v, src & 63, file, line); }
template <typename T> static inline T __shfl_up(T v, unsigned off, int width = 64, PK_SIM_SITE) { (void)width; return pk_sim::shfl(v, (pk_sim::cur_lane() & 63) - (int)off, file, line); }
template <typename T> static inline T __shfl_down(T v, unsigned off, int width = 64, PK_SIM_SITE) { (void)width; return pk_sim::shfl(v, (pk_sim::cur_lane() & 63) + (int)off, file, line); }
template <typename T> static inline T __shfl_xor(T v, int mask, int width = 64, PK_SIM_SITE) { (void)width; return pk_sim::shfl(v, ((pk_sim::cur_lane() & 63) ^ mask) & 63, file, line); }
// v_mov_b32_dpp for the controls pk::wave_excl_scan (pk_device.hpp) uses, as in wave_shim.h: row_shr:1..15, row_bcast:15, row_bcast:31
static inline int __builtin_amdgcn_update_dpp(int old, int src, int ctrl, int row_mask, int bank_mask, bool bound_ctrl, PK_SIM_SITE) {
    const int w = pk_sim::meet(pk_sim::K_SHFL, (uint32_t)src, file, line), l = pk_sim::cur_lane() & 63;
    int from = -1;
    bool in_range = true;
    if (ctrl >= 0x111 && ctrl <= 0x11f) { from = l - (ctrl - 0x110); in_range = (l & 15) >= ctrl - 0x110; }
    else if (ctrl == 0x142) { from = (l & ~15) - 1; in_range = l >= 16; }
    else if (ctrl == 0x143) { from = 31; in_range = l >= 32; }
    else { fprintf(stderr, "wg_sim: update_dpp control 0x%x is not implemented\n", ctrl); abort(); }
    if (!((row_mask >> (l >> 4)) & 1) || !((bank_mask >> ((l >> 2) & 3)) & 1)) return old;
    if (!in_range || !((pk_sim::wave_mask(w) >> from) & 1)) return bound_ctrl ? 0 : old;
    return (int)(uint32_t)pk_sim::wave_val(w, from);
}
// lanes below this one among the mask's bits (v_mbcnt_lo / _hi_u32_b32)
static inline unsigned __builtin_amdgcn_mbcnt_lo(unsigned mask, unsigned v) {
    const int l = pk_sim::cur_lane() & 63;
    return v + (unsigned)__builtin_popcount(l >= 32 ? mask : (mask & ((1u << l) - 1u)));
}
static inline unsigned __builtin_amdgcn_mbcnt_hi(unsigned mask, unsigned v) {
    const int l = pk_sim::cur_lane() & 63;
    return v + (unsigned)__builtin_popcount(l <= 32 ? 0u : (mask & ((1u << (l - 32)) - 1u)));
}
static inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
