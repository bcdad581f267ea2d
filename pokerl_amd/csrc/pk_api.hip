// pk_api.hip -- host side of the C ABI (include/pokerl_hip.h) of libpokerl_hip.so; kernels: pk_table_kernels.hpp, pk_util_kernels.hpp.  gfx950 only; plain HIP runtime,
// no torch types.  Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC (see pokerl_amd/build.py).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "pk_device.hpp"
#include "pk_table_kernels.hpp"
#include "pk_util_kernels.hpp"
#include "pk_equity.hpp"
#include "pk_equity_ev.hpp"
#include "pk_equity_sampled.hpp"
#include "pk_equity_ranged.hpp"
#include "pk_ev_ranged.hpp"
#include "pk_equity_range.hpp"
#include "pk_equity_rvr.hpp"
#include "pk_river_solver.hpp"
#include "pk_turn_solver.hpp"
#include "pk_equity_hist.hpp"
#include "pk_equity_hist_hero.hpp"
#include "pk_hist_cluster.hpp"
#include "pk_preflop.hpp"
#include "pk_preflop_solver.hpp"
#include "pk_snapshot.hpp"

using namespace pk;

// ================================================================================================ host side
static thread_local std::string g_err;
// The error of a call without a handle (pk_last_error(NULL)): `what`, and the HIP error if there is one.
static int g_fail(int code, const char *what, hipError_t e = hipSuccess) {
    g_err = what;
    if (e != hipSuccess) { g_err += ": "; g_err += hipGetErrorString(e); }
    return code;
}
// An integer knob from the environment: its value if it is set and lies in [lo, hi], otherwise `fallback`.
static int env_int(const char *name, int lo, int hi, int fallback) {
    const char *s = getenv(name);
    if (!s) return fallback;
    const int v = atoi(s);
    return v >= lo && v <= hi ? v : fallback;
}

// A per-device cache of device memory (the stream pool's canary, the judger's scratch arena, the evaluator table) outlives its allocation when the
// application resets the device: a kernel launched on such a pointer would fault, a pooled stream handle dangles.  The seat belt: look the ADDRESS
// up before trusting it -- hipMemGetAddressRange looks it up in the runtime's allocation map, no dereference of a dead object.  The allocator hands
// the same addresses out again after a reset (measured: the evaluator table's address came back as the next handle's arena), so base AND size must
// match -- and every cached allocation has an odd size (PK_ODD_BYTES more than it needs) that no caller is likely to ask for.  Not impossible, so
// pk_stream_pool_drain before hipDeviceReset remains the rule.
#define PK_ODD_BYTES 272
namespace {   // (helpers of this file: no symbols of theirs in the library)
// A grow-only device buffer that outlives the call: THE way to device memory besides a handle's arena.  Each user keeps its own lock,
// stream and head-room rule (`grow_to`: the capacity to allocate when `bytes` do not fit).
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t err = hipSuccess;   // of the last allocation
    // `queued`: the stream whose work may still use the old buffer -- waited for before that is freed.  cache: a per-device cache (above),
    // forgotten and not freed once the device was reset.  NULL: out of memory (the sticky HIP error cleared), and the buffer is empty.
    void *reserve(size_t bytes, size_t grow_to, hipStream_t queued, bool cache = false) {
        if (cache && !alive()) *this = DevBuf{};
        if (p && cap >= bytes) return p;
        if (p && hipStreamSynchronize(queued) != hipSuccess) (void)hipGetLastError();
        drop();
        err = hipMalloc(&p, grow_to + (cache ? PK_ODD_BYTES : 0));
        if (err != hipSuccess) { (void)hipGetLastError(); p = nullptr; return nullptr; }
        cap = grow_to;
        return p;
    }
    bool alive() const {   // a per-device cache: it is allocated, and the allocation still exists
        if (!p) return false;
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        const hipError_t e = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p);
        if (e != hipSuccess) (void)hipGetLastError();
        return e == hipSuccess && (const void *)base == p && size == cap + PK_ODD_BYTES;
    }
    void drop() {   // frees without waiting for a stream (hipFree waits for the device)
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
    }
};
// the head room of the per-device caches: at least 1 MiB, else 1/div more than asked for
static inline size_t with_headroom(size_t bytes, int div) { return bytes < (1u << 20) ? (1u << 20) : bytes + bytes / div; }
// Staging of a call on host arrays in ONE device buffer: name the pieces (each 256-byte aligned), reserve `total` bytes, set `base`, then
// upload(), launch on at<T>(piece), download() -- or run(), which is the three.  An optional array the caller left out (in / out with a
// NULL host pointer) gets no piece: at() gives the kernel NULL for it, and nothing is copied.
struct Stage {
    struct Piece { size_t off, bytes; const void *src; void *dst; };
    std::vector<Piece> pieces;
    size_t total = 0;
    char *base = nullptr;
    int add(size_t bytes, const void *src = nullptr, void *dst = nullptr) {   // src: host array to upload from, dst: to download into
        pieces.push_back(Piece{total, bytes, src, dst});
        total += (bytes + 255) & ~(size_t)255;
        return (int)pieces.size() - 1;
    }
    int in(const void *host, size_t bytes) { return host ? add(bytes, host) : -1; }
    int out(void *host, size_t bytes) { return host ? add(bytes, nullptr, host) : -1; }
    int inout(void *host, size_t bytes) { return host ? add(bytes, host, host) : -1; }   // uploaded, then downloaded into the same array
    template <typename T> T *at(int piece) const { return piece < 0 ? nullptr : (T *)(base + pieces[(size_t)piece].off); }
    // The copies are queued on `stream` up to the first HIP error; download() then waits for the stream.
    hipError_t upload(hipStream_t stream) const {
        hipError_t e = hipSuccess;
        for (const Piece &c : pieces)
            if (e == hipSuccess && c.src && c.bytes) e = hipMemcpyAsync(base + c.off, c.src, c.bytes, hipMemcpyHostToDevice, stream);
        return e;
    }
    hipError_t download(hipStream_t stream) const {
        hipError_t e = hipSuccess;
        for (const Piece &c : pieces)
            if (e == hipSuccess && c.dst && c.bytes) e = hipMemcpyAsync(c.dst, base + c.off, c.bytes, hipMemcpyDeviceToHost, stream);
        return e == hipSuccess ? hipStreamSynchronize(stream) : e;
    }
    template <typename F> hipError_t run(hipStream_t stream, F launch) const {   // launch(): queues the kernels, returns their HIP error
        hipError_t e = upload(stream);
        if (e == hipSuccess) e = launch();
        return e == hipSuccess ? download(stream) : e;
    }
};
// The count outputs an equity call on host arrays wants, as pieces of its staging
struct EqStagedOut {
    int win, tie, share, boards, status;
    EqStagedOut(Stage &g, int N, size_t m, uint32_t *win, uint32_t *tie, uint64_t *share, uint32_t *boards, uint8_t *status)
        : win(g.out(win, m * N * 4)), tie(g.out(tie, m * N * 4)), share(g.out(share, m * N * 8)), boards(g.out(boards, m * 4)), status(g.out(status, m)) {}
    EqOut at(const Stage &g) const { return EqOut{g.at<uint32_t>(win), g.at<uint32_t>(tie), g.at<uint64_t>(share), g.at<uint32_t>(boards), g.at<uint8_t>(status)}; }
};
// ... and a range-equity call
struct EqrStagedOut {
    int agg, win, tie, boards, status;
    EqrStagedOut(Stage &g, size_t m, uint64_t *agg, uint32_t *win, uint32_t *tie, uint32_t *boards, uint8_t *status)
        : agg(g.out(agg, m * 3 * 8)), win(g.out(win, m * EQR_HOLDINGS * 4)), tie(g.out(tie, m * EQR_HOLDINGS * 4)), boards(g.out(boards, m * 4)),
          status(g.out(status, m)) {}
    EqrOut at(const Stage &g) const { return EqrOut{g.at<uint64_t>(agg), g.at<uint32_t>(win), g.at<uint32_t>(tie), g.at<uint32_t>(boards), g.at<uint8_t>(status)}; }
};
// ... and a range-against-range call
struct RvrStagedOut {
    int win, tie, tot, boards, status;
    RvrStagedOut(Stage &g, size_t m, uint64_t *win, uint64_t *tie, uint64_t *tot, uint32_t *boards, uint8_t *status)
        : win(g.out(win, m * RVR_HOLDINGS * 8)), tie(g.out(tie, m * RVR_HOLDINGS * 8)), tot(g.out(tot, m * RVR_HOLDINGS * 8)), boards(g.out(boards, m * 4)),
          status(g.out(status, m)) {}
    RvrOut at(const Stage &g) const { return RvrOut{g.at<uint64_t>(win), g.at<uint64_t>(tie), g.at<uint64_t>(tot), g.at<uint32_t>(boards), g.at<uint8_t>(status)}; }
};
// ... and a strength-histogram call
struct HistStagedOut {
    int hist, void_, completions, status;
    HistStagedOut(Stage &g, size_t m, int nbins, uint16_t *hist, uint16_t *void_, uint32_t *completions, uint8_t *status)
        : hist(g.out(hist, m * RVR_HOLDINGS * (size_t)nbins * 2)), void_(g.out(void_, m * RVR_HOLDINGS * 2)), completions(g.out(completions, m * 4)),
          status(g.out(status, m)) {}
    HistOut at(const Stage &g) const { return HistOut{g.at<uint16_t>(hist), g.at<uint16_t>(void_), g.at<uint32_t>(completions), g.at<uint8_t>(status)}; }
};
// ... and a hero-histogram call, with the bucket stage's centroids, labels and distances
struct HeroHistStaged {
    int hist, void_, completions, status, centroids, label, dist, K;
    HeroHistStaged(Stage &g, size_t m, int nbins, uint16_t *hist, uint16_t *void_, uint32_t *completions, uint8_t *status, int K, const uint16_t *centroids,
                   uint16_t *label, uint32_t *dist)
        : hist(g.out(hist, m * (size_t)nbins * 2)), void_(g.out(void_, m * 2)), completions(g.out(completions, m * 4)), status(g.out(status, m)),
          centroids(K > 0 ? g.in(centroids, (size_t)K * nbins * 2) : -1), label(g.out(label, m * 2)), dist(g.out(dist, m * 4)), K(K) {}
    HeroHistOut at(const Stage &g) const { return HeroHistOut{g.at<uint16_t>(hist), g.at<uint16_t>(void_), g.at<uint32_t>(completions), g.at<uint8_t>(status)}; }
    HeroHistBucket bucket(const Stage &g) const { return HeroHistBucket{K, g.at<uint16_t>(centroids), g.at<uint16_t>(label), g.at<uint32_t>(dist)}; }
};
}  // namespace

struct pk_handle {
    int device = 0, T = 0, N = 0, dealer = 0;
    int tpb = 64;   // tables per wavefront (Hot::tpb)
    int env_tpb = 64;  // ... of the PokerGameEnv kernels (hot_env): see pk_create; knob PK_ENV_TPB
    Hot hot_env{};
    bool occ3 = false;  // k_rollout_occ3 (registers capped for 3 waves per SIMD) vs k_rollout: see pk_create; knob PK_OCC3
    int tab_min_steps = 16;  // k_rollout_tab for launches of at least this many steps (0: never; 20-step launches: no gain, no loss); knob PK_ROLLOUT_TAB
    // lanes parked at end_hand before a wave runs end_block (the kernels look every 4 betting passes); knob PK_PARK /
    // pk_set_tuning.  0 = the measured optimum of each kernel: 28 for k_rollout with random agents (20.9 vs 20.6 G at
    // 20-step launches, the same at long ones), 32 for the all-in agents (44.3 vs 43.3 G) and for the env kernels.
    int park = 0;
    int endk = 48;  // a deferred rollout launch ends once fewer than this many of a wave's lanes have work; knob PK_ENDK
                    // (measured optimum 44..52 at 20 and at 512 steps per launch: tools/tune_sweep.py)
    // Deferred rollout work: steps requested by pk_rollout that no launch has executed yet may exist on the device
    // (State::owed, steps in flight).  Every entry point that reads or changes table state flushes first.
    bool pending = false;
    int pend_policy = 0, pend_auto = 0;
    // Host-side coalescing of asynchronous pk_rollout calls (counters == NULL, auto_reset): while the two most recent
    // launches are still running, a call only ADDS its steps to `acc`; they are launched as ONE kernel once a launch slot
    // frees up, at `coalesce` accumulated steps, or by the flush every observer issues.  A stream of 20-step calls thus
    // runs as launches of up to `coalesce` steps: the fixed cost of a launch (load + store of every table, ramp and
    // tail: ~8 us of a 60 us 20-step launch) is paid once per launch, not per call.  0: every call launches.
    int coalesce = 1024;
    int acc = 0;
    hipEvent_t ev_ring[2] = {nullptr, nullptr};
    bool ev_used[2] = {false, false};
    int ev_idx = 0;
    // launches of the fused rollout kernel since pk_get_launch_stats(reset): count, steps summed, min / max steps per launch
    uint64_t st_launches = 0, st_steps = 0, st_min = 0, st_max = 0;
    int env_seat0 = 0, env_opp = 0, env_auto = 0;   // agents / auto_reset of the PokerGameEnv.steps in flight (env_pending)
    // Sub-batches of pk_env_step_async_d inside ONE handle (pk_set_env_batches): contiguous table ranges, each on its own
    // internal stream, launched round robin -- a call launches one range and delivers the range launched longest ago, so that
    // the launches of the ranges overlap like those of separate handles do (a launch ends with a tail; launches on one stream
    // are serialised).
    int env_batches = 1, env_range = 0;             // number of ranges, tables per range (a multiple of 64)
    hipStream_t env_streams[PK_MAX_ENV_BATCHES] = {};
    hipEvent_t env_done[PK_MAX_ENV_BATCHES] = {};
    bool env_launched[PK_MAX_ENV_BATCHES] = {};
    hipEvent_t env_in = nullptr;
    int env_next = 0, env_last_begin = 0, env_last_end = 0, env_last_fresh = 0;
    bool env_multi = false;                         // ... they belong to pk_env_step_multi_d, with these per-seat agents:
    uint64_t env_seats = 0;
    // PokerGameEnv.steps left in flight by pk_env_step_async_d (State::env_ctx): every other entry point that touches
    // table state refuses to run until a draining call (max_passes <= 0) has completed them.
    bool env_pending = false;
    bool step_pending = false;   // Game.steps left in flight by pk_step_async_d (their machine state is in the tables' cursor bits): as env_pending
    int step_auto = 0;
    bool host_step = false;   // between pk_env_step_begin and pk_env_step_end: the caller's host buffers are the targets of queued copies
    hipStream_t stream = nullptr, own_stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    State S{};
    State *d_S = nullptr;  // device copy of S (kernels that take the state by pointer)
    Hot hot{};             // loop scalars, passed by value
    unsigned long long *d_totals = nullptr;  // [PK_NUM_COUNTERS] output of k_sum_counters
    void *arena = nullptr;
    // staging (device) + pinned staging (host) of the host-buffer entry points
    int32_t *d_actions = nullptr;
    uint8_t *d_flags = nullptr, *d_terr = nullptr, *d_mask = nullptr, *d_done = nullptr, *d_handf = nullptr;
    double *d_reward = nullptr;
    void *d_export = nullptr;
    size_t export_bytes = 0;
    uint8_t *h_pinned = nullptr;  // [T] pinned: per-table error bytes of pk_step / pk_env_step
    DevBuf d_obs_packed;                 // [T][PK_OBS_PACKED_BYTES(N)]: device staging of pk_env_step_begin (allocated on first use)
    uint8_t *env_obs_packed = nullptr;   // pk_set_env_obs_packed: device buffer [T][PK_OBS_PACKED_BYTES(N)] or NULL
    double *step_obs = nullptr;          // pk_set_step_obs: device buffers the Game.step kernels write the row of the player to act into, or NULL
    uint8_t *step_obs_packed = nullptr;
    // snapshots (pk_save_tables_d ...), allocated on first use: the refusal word the check kernels write, one count per table for the
    // duplicate / overlap checks of destination indices, a grow-only staging buffer (host-memory calls, overlapping clones) and the event
    // that orders a clone between two handles' streams
    uint32_t *snap_word = nullptr, *snap_mark = nullptr;
    DevBuf snap_stage;
    hipEvent_t snap_ev = nullptr;
    std::string err;
    int fail(int code, const char *what, hipError_t e = hipSuccess) {
        g_fail(code, what, e);
        err = g_err;
        return code;
    }
};

// Entry points run on the handle's device but leave the caller's current device as they found it (a host
// application may be driving other GPUs, e.g. through torch, from the same thread).
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define ON_DEVICE(h)                                             \
    DeviceGuard guard_((h)->device);                             \
    if (!guard_.ok) return (h)->fail(PK_E_HIP, "hipSetDevice")

#define HIPCHK(h, call)                                            \
    do {                                                           \
        hipError_t e_ = (call);                                    \
        if (e_ != hipSuccess) return (h)->fail(PK_E_HIP, #call, e_); \
    } while (0)

// One instantiation of every table kernel per seat count, PK_MIN_PLAYERS .. PK_MAX_PLAYERS, each seat count compiled in a
// translation unit of its own (pk_tables.hip).  A development build may hold ONE seat count (-DPK_ONLY_SEATS=N: seconds
// instead of minutes); pk_create refuses the others there.
#ifdef PK_ONLY_SEATS
#define PK_SEAT_ENABLED(N) ((N) == (PK_ONLY_SEATS))
#else
#define PK_SEAT_ENABLED(N) 1
#endif
#define PK_FOR_SEATS_LE10(X) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10)
#define PK_FOR_SEATS_GT10(X) X(11) X(12) X(13) X(14) X(15) X(16)
#define PK_FOR_SEATS_LE6(X) X(2) X(3) X(4) X(5) X(6)
static_assert(PK_MIN_PLAYERS == 2 && PK_MAX_PLAYERS == 16, "the lists above name the seat counts");
#define PK_DECLARE_ALL(N) PK_TABLE_KERNELS(PK_DECLARE_KERNEL, N)
#define PK_DECLARE_ALL_LE10(N) PK_TABLE_KERNELS_LE10(PK_DECLARE_KERNEL, N)
#define PK_DECLARE_ALL_LE6(N) PK_TABLE_KERNELS_LE6(PK_DECLARE_KERNEL, N)
PK_FOR_SEATS_LE10(PK_DECLARE_ALL)
PK_FOR_SEATS_GT10(PK_DECLARE_ALL)
PK_FOR_SEATS_LE10(PK_DECLARE_ALL_LE10)
PK_FOR_SEATS_LE6(PK_DECLARE_ALL_LE6)

// The seat-count dispatch: calls launch(std::integral_constant<int, N>{}) for N == n if this build holds seat count n and n <= MAX
// (16; 10 for the 168-register kernels, which would spill beyond ten seats; 6 for k_rollout_tab).  false: no kernel, nothing launched.
// Only the seat counts the walk reaches are named, so a kernel that does not exist for a seat count is never referenced.
template <int MAX = PK_MAX_PLAYERS, int N = PK_MIN_PLAYERS, typename F>
static bool seat_dispatch(int n, F &&launch) {
    if constexpr (N > MAX) {
        return false;
    } else {
        if constexpr (PK_SEAT_ENABLED(N)) {
            if (n == N) { launch(std::integral_constant<int, N>{}); return true; }
        }
        return seat_dispatch<MAX, N + 1>(n, launch);
    }
}
// The launch of KERNEL<N> that seat_dispatch calls: one wavefront per workgroup
#define SEAT_KERNEL(KERNEL, grid, stream, ...) \
    [&](auto n_) { hipLaunchKernelGGL(KERNEL<decltype(n_)::value>, dim3(grid), dim3(PK_TABLE_BLOCK), 0, (stream), __VA_ARGS__); }
// ... for the handle's seat count, checked
template <int MAX = PK_MAX_PLAYERS, typename F>
static int seat_launch(pk_handle *h, F &&launch) {
    if (!seat_dispatch<MAX>(h->N, launch)) return h->fail(PK_E_INVALID_ARG, "no kernel for this seat count in this build of the library");
    HIPCHK(h, hipGetLastError());
    return PK_OK;
}

#define PK_STR_(x) #x
#define PK_STR(x) PK_STR_(x)
static inline bool bad_policy(int policy) { return policy < 0 || policy >= PK_NUM_POLICIES; }
// every seat plays `policy`: the per-seat word of the entry points that take ONE opponent policy
static inline uint64_t uniform_seats(int policy) { return 0x1111111111111111ull * (uint64_t)(policy & 15); }
static inline int table_grid(const pk_handle *h) { return (h->T + h->tpb - 1) / h->tpb; }
// parking threshold for waves that hold h->tpb tables instead of 64
static inline int scaled_park(const pk_handle *h, int dflt = 32, int tpb = 0) {
    int p = ((h->park > 0 ? h->park : dflt) * (tpb > 0 ? tpb : h->tpb) + 63) / 64;
    return p < 1 ? 1 : p;
}
static inline int env_grid(const pk_handle *h) { return (h->T + h->env_tpb - 1) / h->env_tpb; }
// (16: asynchronous env.step +1.3 % over 32 with the round's final kernels, synchronous unchanged; 12 the same, 24 half of it)
static inline int env_park(const pk_handle *h) { return scaled_park(h, 16, h->env_tpb); }
static inline int flat_grid(size_t n) { return (int)((n + 255) / 256); }
// the observation getters: one table per lane, 64-thread workgroups -- 65 536 tables are 1 024 waves, one per SIMD (256-thread blocks put them on a quarter of the CUs' schedulers' slots)
#define OBS_BLOCK 64
static inline int obs_grid(int T) { return (T + OBS_BLOCK - 1) / OBS_BLOCK; }

// One fused rollout launch: every table owes k_steps more steps; the launch ends once fewer than `endk` lanes of a
// wave have work left (endk == 1: runs to completion).
static int launch_rollout(pk_handle *h, int k_steps, int policy, int auto_reset, int endk) {
    const int slack = endk <= 1 ? PK_WAVE : ((PK_WAVE - endk) * h->tpb) / PK_WAVE;   // lanes allowed to idle before a launch ends
    const int park = scaled_park(h, policy == PK_POLICY_RANDOM ? 28 : 32), clear_terr = h->pending ? 0 : 1;
#define ROLLOUT(KERNEL) SEAT_KERNEL(KERNEL, table_grid(h), h->stream, (const State *)h->d_S, h->hot, k_steps, auto_reset, park, slack, clear_terr)
    int rc;
    if (policy == PK_POLICY_RANDOM && k_steps == 1 && endk <= 1 && !h->occ3) rc = seat_launch(h, ROLLOUT(k_rollout_single));
    else if (policy == PK_POLICY_CALL) rc = seat_launch(h, ROLLOUT(k_rollout_call));
    else if (!h->occ3) {
        // k_rollout_tab: the showdown hands ranked by the table-driven evaluator -- where its 40 KB of LDS per wave cost no occupancy (at most one
        // wave per SIMD: 1 024 workgroups) and the launch is long enough to pay for staging the table (~1.5 us); knob PK_ROLLOUT_TAB (min steps, 0 = off)
        const bool tab_ok = h->S.evtab && h->tab_min_steps > 0 && k_steps >= h->tab_min_steps && table_grid(h) <= 1024;
        if (policy == PK_POLICY_RANDOM && h->N <= 6 && tab_ok) rc = seat_launch<6>(h, ROLLOUT(k_rollout_tab));
        else if (policy == PK_POLICY_ALLIN && h->N <= 10 && tab_ok) rc = seat_launch<10>(h, ROLLOUT(k_rollout_allin_tab));   // (no action ring in LDS: up to ten seats)
        else if (policy == PK_POLICY_RANDOM) rc = seat_launch(h, ROLLOUT(k_rollout));
        else rc = seat_launch(h, ROLLOUT(k_rollout_allin));
    } else {
        if (policy == PK_POLICY_RANDOM) rc = seat_launch<10>(h, ROLLOUT(k_rollout_occ3));
        else rc = seat_launch<10>(h, ROLLOUT(k_rollout_occ3_allin));
    }
#undef ROLLOUT
    if (rc) return rc;
    h->pending = slack < PK_WAVE;
    h->pend_policy = policy; h->pend_auto = auto_reset;
    h->st_launches += 1; h->st_steps += (uint64_t)k_steps;
    if (k_steps > 0) {
        h->st_min = (h->st_min == 0 || (uint64_t)k_steps < h->st_min) ? (uint64_t)k_steps : h->st_min;
        h->st_max = (uint64_t)k_steps > h->st_max ? (uint64_t)k_steps : h->st_max;
    }
    return PK_OK;
}
// Completes whatever deferred rollout launches left undone.  Called by every entry point that reads or mutates tables.
static int flush_rollout(pk_handle *h) {
    if (!h->pending && h->acc == 0) return PK_OK;
    const int k = h->acc;
    h->acc = 0;
    return launch_rollout(h, k, h->pend_policy, h->pend_auto, 1);
}
// One asynchronous, deferring launch of the accumulated steps; remembers it in the two-slot event ring.
static int launch_coalesced(pk_handle *h, int policy, int auto_reset) {
    const int k = h->acc;
    h->acc = 0;
    int rc = launch_rollout(h, k, policy, auto_reset, h->endk);
    if (rc) return rc;
    HIPCHK(h, hipEventRecord(h->ev_ring[h->ev_idx], h->stream));
    h->ev_used[h->ev_idx] = true;
    h->ev_idx ^= 1;
    return PK_OK;
}
static inline bool in_flight(const pk_handle *h) { return h->env_pending || h->host_step || h->step_pending; }
static int flush(pk_handle *h) {
    if (h->step_pending)
        return h->fail(PK_E_BUSY, "Game.steps are in flight (pk_step_async_d): drain them with max_hands = 0 first");
    if (h->host_step)
        return h->fail(PK_E_BUSY, "a pk_env_step_begin is waiting for its pk_env_step_end: the copies into the caller's buffers are still queued");
    if (h->env_pending)
        return h->fail(PK_E_BUSY, "PokerGameEnv steps are in flight (pk_env_step_async_d / pk_env_step_multi_d): drain them with max_passes = 0 "
                                  "(pk_env_end_multi_d where seats are played by the caller) first");
    return flush_rollout(h);
}
#define FLUSH(h)                   \
    do {                           \
        int rc_ = flush(h);        \
        if (rc_) return rc_;       \
    } while (0)
// The device-resident READERS (pk_pick_actions_d, pk_get_obs_d, pk_get_obs_packed_d, pk_get_valid_actions_d, pk_get_f64_d) also work while
// Game.steps are in flight (pk_step_async_d): a caller needs them to act on the tables that are ready.  What they return for a table whose
// step is still in flight is that table in the middle of its step -- ready_d says which rows to ignore.
static int flush_reader(pk_handle *h) {
    if (h->step_pending && !h->env_pending && !h->host_step) return PK_OK;
    return flush(h);
}
#define FLUSH_READER(h)                \
    do {                               \
        int rc_ = flush_reader(h);     \
        if (rc_) return rc_;           \
    } while (0)

template <typename F>
static int export_to_host(pk_handle *h, void *out, size_t bytes, F launch) {
    ON_DEVICE(h);
    FLUSH(h);
    if (bytes > h->export_bytes) return h->fail(PK_E_INVALID_ARG, "export buffer too small");
    launch();
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, h->d_export, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PK_OK;
}

// Streams are RECYCLED through a per-device pool instead of being destroyed with their handle: a process that opens and closes
// handles (bench.py's legs, a test suite) keeps working on the same few streams -- and therefore on the same hardware queues --
// instead of walking through HIP's stream-to-queue assignment (see the sub-batch notes below and docs/history.md section 5).
static std::mutex g_stream_mu;
static std::vector<hipStream_t> g_stream_pool[PK_MAX_DEVICES][2];   // [device][0: normal priority, 1: the sub-batch streams]
// The internal streams of pk_set_env_batches are created with the HIGHEST stream priority: HIP keeps separate hardware queues per
// priority level, so they do not compete for the four normal-priority queues with the caller's stream, the legacy default stream
// (one hipMemcpy or one torch kernel brings it to life) and whatever else the process has created -- with normal-priority streams a
// process that had merely made one hipMemcpy before creating the handle ran 524 288 x 6 in three sub-batches at 2.57 G env.step/s
// against 3.66 G (tools/env_queue_scenarios.py).  env PK_ENV_STREAM_PRIO=0: off.
static int pool_class(bool sub_batch) {
    static const bool prio = env_int("PK_ENV_STREAM_PRIO", INT_MIN, INT_MAX, 1) != 0;
    return (sub_batch && prio) ? 1 : 0;
}
// How the pool notices a device reset WITHOUT touching a pooled (then dangling) stream handle: a small device allocation made when the first stream
// of a device is pooled.
static DevBuf g_pool_canary[PK_MAX_DEVICES];
static bool pool_alive(int device) {   // caller holds g_stream_mu and has the device current
    const bool ok = g_pool_canary[device].alive();
    if (!ok) g_pool_canary[device] = DevBuf{};          // (not freed: it no longer exists)
    return ok;
}
static hipError_t stream_acquire(int device, hipStream_t *out, bool sub_batch = false) {   // the device is current
    const int cls = pool_class(sub_batch);
    if (device >= 0 && device < PK_MAX_DEVICES) {
        std::lock_guard<std::mutex> lock(g_stream_mu);
        auto &pool = g_stream_pool[device][cls];
        if (!pool.empty() && !pool_alive(device)) {
            // The application reset the device (hipDeviceReset destroys every stream) without pk_stream_pool_drain: the pooled handles are
            // dangling pointers -- ANY call on one, hipStreamQuery included, segfaults inside the runtime (measured, ROCm 7.2).  Forget them
            // (nothing is left to destroy) and create a fresh stream below.
            for (int c = 0; c < 2; ++c) g_stream_pool[device][c].clear();
        }
        if (!pool.empty()) { *out = pool.back(); pool.pop_back(); return hipSuccess; }
    }
    if (cls == 1) {
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least)
            return hipStreamCreateWithPriority(out, hipStreamNonBlocking, greatest);
        (void)hipGetLastError();
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}
static void stream_release(int device, hipStream_t s, bool sub_batch = false) {   // the device is current; s is idle or about to be
    if (!s) return;
    if (hipStreamSynchronize(s) != hipSuccess) {      // a stream that cannot even be waited for (stale after a device reset, or broken) is not recycled
        (void)hipGetLastError(); (void)hipStreamDestroy(s); (void)hipGetLastError();
        return;
    }
    if (device >= 0 && device < PK_MAX_DEVICES) {
        std::lock_guard<std::mutex> lock(g_stream_mu);
        if (!g_pool_canary[device].p) {                // the pool's reset detector (pool_alive); without one the stream is not pooled
            for (int c = 0; c < 2; ++c) g_stream_pool[device][c].clear();    // (whatever was pooled under an earlier, vanished canary is stale)
            if (!g_pool_canary[device].reserve(4096, 4096, s, true)) { (void)hipStreamDestroy(s); return; }
        }
        g_stream_pool[device][pool_class(sub_batch)].push_back(s);
    } else (void)hipStreamDestroy(s);
}

// Destroys the pooled (idle) streams of a device; -1: of every device.  For a host application that resets the device (hipDeviceReset
// invalidates every stream, pooled ones included) or wants its hardware queues back.  Streams of live handles are not in the pool.
static int drain_stream_pool(int device) {
    std::lock_guard<std::mutex> lock(g_stream_mu);
    int n = 0;
    for (int d = 0; d < PK_MAX_DEVICES; ++d) {
        if (device >= 0 && d != device) continue;
        for (int cls = 0; cls < 2; ++cls) {
            auto &pool = g_stream_pool[d][cls];
            if (pool.empty()) continue;
            DeviceGuard guard(d);
            const bool alive = guard.ok && pool_alive(d);     // (after a device reset the handles are dangling: dropped, not destroyed)
            for (hipStream_t s : pool) { if (alive) (void)hipStreamDestroy(s); ++n; }
            (void)hipGetLastError();
            pool.clear();
        }
        if (g_pool_canary[d].p && g_stream_pool[d][0].empty() && g_stream_pool[d][1].empty()) {
            DeviceGuard guard(d);
            if (guard.ok && pool_alive(d)) g_pool_canary[d].drop();
            (void)hipGetLastError();
            g_pool_canary[d] = DevBuf{};
        }
    }
    return n;
}

// Is there a HIP device at all (PK_E_NO_DEVICE), and is `device` one of them and below `limit` (PK_E_INVALID_ARG)?  Device 0: any device.
static int check_device(const char *call, int device, int limit = INT_MAX) {
    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return g_fail(PK_E_NO_DEVICE, (std::string(call) + ": no HIP device available (" + (e != hipSuccess ? hipGetErrorString(e) : "0 devices") +
                                       "); this library has no CPU fallback").c_str());
    if (device < 0 || device >= ndev || device >= limit) return g_fail(PK_E_INVALID_ARG, (std::string(call) + ": device index out of range").c_str());
    return PK_OK;
}
// ON_DEVICE of the calls without a handle: the device check, then `device` current until the call returns
#define ON_DEVICE_INDEX(call, device, limit)                                     \
    if (int rc_ = check_device(call, device, limit)) return rc_;                 \
    DeviceGuard guard_(device);                                                  \
    if (!guard_.ok) return g_fail(PK_E_HIP, (std::string(call) + ": hipSetDevice failed").c_str())

// The argument block of the PokerGameEnv.step kernels (pk_table_kernels.hpp EnvKernArgs): common fields; callers set the rest.
static EnvKernArgs env_args(const pk_handle *h, const int32_t *actions_d, int seat0_policy, uint64_t seatpol, int auto_reset,
                            double *reward_d, uint8_t *done_d, uint8_t *hand_d, uint8_t *terr_d, double *obs_d) {
    EnvKernArgs ka{};
    ka.Sp = (const State *)h->d_S; ka.H = h->hot_env;
    ka.A.actions = actions_d; ka.A.seat0_policy = seat0_policy; ka.A.seatpol = seatpol; ka.A.auto_reset = auto_reset;
    ka.A.reward = reward_d; ka.A.done = done_d; ka.A.hand = hand_d; ka.A.terr = terr_d; ka.A.obs = obs_d;
    ka.A.obs_packed = nullptr;             // (pk_set_env_obs_packed's buffer: set by the three entry points the header names, see with_packed)
    ka.A.park = env_park(h); ka.A.t0 = 0; ka.A.tend = h->T;
    return ka;
}

// pk_set_env_obs_packed: pk_env_step_fused_d / _async_d / _multi_d write the compact row of every table they deliver
static inline EnvKernArgs with_packed(const pk_handle *h, EnvKernArgs ka) { ka.A.obs_packed = h->env_obs_packed; return ka; }

// the table-driven evaluator's rank-mask table, one per device (defined with the judger entry points); built on `stream` the first time
static const uint32_t *eval7_table(int device, hipStream_t stream = nullptr);

extern "C" {

int pk_abi_version(void) { return PK_ABI_VERSION; }

#ifndef PK_SOURCE_HASH
#define PK_SOURCE_HASH "unknown"
#endif
const char *pk_build_info(void) { return "abi=" PK_STR(PK_ABI_VERSION) " src=" PK_SOURCE_HASH; }

int pk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *pk_last_error(const pk_handle *h) { return h ? h->err.c_str() : g_err.c_str(); }

int pk_create(pk_handle **out, int device, int num_tables, int num_players, const double *start_credits,
              double start_credit_scalar, double big_blind, double small_blind, int dealer, uint64_t seed,
              uint32_t table_id_base) {
    if (!out) { g_err = "pk_create: out is NULL"; return PK_E_INVALID_ARG; }
    *out = nullptr;
    if (num_tables < 1 || num_players < PK_MIN_PLAYERS || num_players > PK_MAX_PLAYERS) {
        g_err = "pk_create: need num_tables >= 1 and " PK_STR(PK_MIN_PLAYERS) " <= num_players <= " PK_STR(PK_MAX_PLAYERS)
                " (the reference takes any num_players, game.py:246; a 17th seat does not fit the 16 nibbles of a policy word, and from 18 seats on "
                "numpy's argsort of the bets, game.py:495, is no longer a stable insertion sort, so the side-pot order among equal bets is not a "
                "rule the reference pins: DESIGN.md section 8, docs/history.md section 9)";
        return PK_E_INVALID_ARG;
    }
    if (!seat_dispatch(num_players, [](auto) {})) { g_err = "pk_create: this development build of the library holds one seat count only (PK_ONLY_SEATS)"; return PK_E_INVALID_ARG; }
    {   // Money must be finite: the library is built with -fno-honor-nans (v_max_f64 / v_min_f64 for np.max / np.minimum), and an
        // infinite stack turns into NaN at the first all-in (inf - inf), where numpy and the device would disagree silently.
        bool finite = std::isfinite(big_blind) && std::isfinite(small_blind);
        if (start_credits) { for (int i = 0; i < num_players; ++i) finite = finite && std::isfinite(start_credits[i]); }
        else finite = finite && std::isfinite(start_credit_scalar);
        if (!finite) { g_err = "pk_create: start_credits, big_blind and small_blind must be finite (no inf / NaN)"; return PK_E_INVALID_ARG; }
    }
    if (int rc = check_device("pk_create", device)) return rc;
    pk_handle *h = new pk_handle();
    h->device = device; h->T = num_tables; h->N = num_players; h->dealer = dealer;
    {   // small batches: spread the tables over all 1 024 SIMDs of the chip (power of two, 1..64 tables per wave)
        int tpb = 64;
        while (tpb > 1 && (long)num_tables <= 1024L * (tpb / 2)) tpb /= 2;
        h->tpb = env_int("PK_TPB", 1, 64, tpb);
        // k_rollout_occ3 (registers capped at 168: three waves per SIMD) only where it was measured to pay: six seats
        // (k_rollout<6> needs 171 registers -- profiles/r04_resource_usage.txt --, the capped build 162 without a spill) as soon as a SIMD gets a
        // third wave, i.e. beyond 131 072 tables; seven seats from 262 144 tables (+6..10 %), eight from 524 288 (+5..7 %).
        // Up to five seats k_rollout fits 168 registers by itself; at nine and ten seats the cap spills to scratch and
        // loses 10..35 % at every batch size.
        const bool occ3 = (num_players == 6 && num_tables > 131072) || (num_players == 7 && num_tables >= 262144) ||
                          (num_players == 8 && num_tables >= 524288);
        h->occ3 = env_int("PK_OCC3", INT_MIN, INT_MAX, occ3) != 0 && num_players <= 10;
    }
    {   // The env kernels are bound by the tail of the slowest table of a wave (a busted seat 0 waits for the end of the game),
        // not by issue slots: half-populated waves halve that tail and bring a second wave to each SIMD
        // (profiles/r03_env_tpb_sweep.txt); knob PK_ENV_TPB: a power of two
        const int v = env_int("PK_ENV_TPB", 1, 64, h->tpb);
        h->env_tpb = (v & (v - 1)) == 0 ? v : h->tpb;
    }
    h->tab_min_steps = env_int("PK_ROLLOUT_TAB", 0, INT_MAX, h->tab_min_steps);
    h->park = env_int("PK_PARK", 1, 64, h->park);
    h->endk = env_int("PK_ENDK", 1, 64, h->endk);
    h->coalesce = env_int("PK_COALESCE", 0, 1 << 20, h->coalesce);
    auto bail = [&](int code) { g_err = h->err; pk_destroy(h); return code; };
    DeviceGuard guard(device);
    if (!guard.ok) return bail(h->fail(PK_E_HIP, "hipSetDevice"));
    if (stream_acquire(device, &h->own_stream) != hipSuccess) {  // (stream_acquire has validated what it took from the pool, or created a fresh one)
        (void)hipGetLastError();
        return bail(h->fail(PK_E_HIP, "hipStreamCreate"));
    }
    h->stream = h->own_stream;
    if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_ring[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_ring[1], hipEventDisableTiming) != hipSuccess) return bail(h->fail(PK_E_HIP, "hipEventCreate"));
    if (hipHostMalloc((void **)&h->h_pinned, (size_t)num_tables, hipHostMallocDefault) != hipSuccess) return bail(h->fail(PK_E_OOM, "hipHostMalloc"));

    const size_t T = (size_t)num_tables, N = (size_t)num_players;
    const size_t K = 5 + 2 * N, W = (K + 3) / 4;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t obs = (size_t)PK_OBS_DIM(N) * 8;
    h->export_bytes = al(T * (obs > N * 8 ? obs : N * 8));
    const size_t nwaves = (T + (size_t)h->tpb - 1) / (size_t)h->tpb;
    State &S = h->S;
    double *d_start = nullptr;
    Fresh *d_fresh = nullptr;
    // ONE description of the arena, run twice: with base == NULL it only measures (the result is the allocation size),
    // then it hands out the pointers -- an array added here cannot be forgotten in a separately kept size expression.
    auto layout = [&](char *base) -> size_t {
        size_t off = 0;
        auto take = [&](size_t bytes) { void *r = base ? (void *)(base + off) : nullptr; off += al(bytes); return r; };
        S.credits = (double *)take(T * N * 8); S.bets = (double *)take(T * N * 8);
        S.pending = (double *)take(T * N * 8); S.payoffs = (double *)take(T * N * 8);
        S.min_raise = (double *)take(T * 8);
        S.seat_states = (uint64_t *)take(T * 8);
        S.hand_serial = (uint64_t *)take(T * 8); S.step_serial = (uint64_t *)take(T * 8);
        S.cursors = (uint32_t *)take(T * 4); S.hand = (int32_t *)take(T * 4);
        S.owed = (uint32_t *)take(T * 4); S.mid = (uint32_t *)take(T * 4);
        S.env_ctx = (uint64_t *)take(T * 8); S.env_rew = (double *)take(T * 8);
        S.cards = (uint32_t *)take(W * T * 4);
        S.show = (uint32_t *)take(N * T * 4);
        S.valid = (uint8_t *)take(T); S.terr = (uint8_t *)take(T);
        S.counters = (unsigned long long *)take(nwaves * PK_NUM_COUNTERS * 8);
        h->d_totals = (unsigned long long *)take(PK_NUM_COUNTERS * 8);
        S.prof = (unsigned long long *)take(PF_SLOTS * 8);
        h->d_S = (State *)take(sizeof(State));
        d_start = (double *)take(PK_MAX_PLAYERS * 8);
        d_fresh = (Fresh *)take(sizeof(Fresh));
        h->d_actions = (int32_t *)take(T * 4);
        h->d_flags = (uint8_t *)take(T); h->d_terr = (uint8_t *)take(T); h->d_mask = (uint8_t *)take(T);
        h->d_done = (uint8_t *)take(T); h->d_handf = (uint8_t *)take(T);
        h->d_reward = (double *)take(T * 8);
        h->d_export = take(h->export_bytes);
        return off;
    };
    const size_t total = layout(nullptr);
    const hipError_t e = hipMalloc(&h->arena, total);
    if (e != hipSuccess) return bail(h->fail(PK_E_OOM, "hipMalloc(table state)", e));
    if (hipMemsetAsync(h->arena, 0, total, h->stream) != hipSuccess) return bail(h->fail(PK_E_HIP, "hipMemset"));
    if (layout((char *)h->arena) != total) return bail(h->fail(PK_E_HIP, "arena layout changed between its two passes"));
    for (int i = 0; i < PK_MAX_PLAYERS; ++i)
        S.start_credits[i] = i < num_players ? (start_credits ? start_credits[i] : start_credit_scalar) : 0.0;
    S.big_blind = big_blind; S.small_blind = small_blind;
    S.key0 = (uint32_t)seed; S.key1 = (uint32_t)(seed >> 32);
    S.table_id_base = table_id_base; S.T = num_tables;
    // k_rollout_tab / k_rollout_allin_tab stage it in LDS (NULL -- out of memory -- : k_rollout(_allin) is used).  Built on the HANDLE's stream: the legacy
    // default stream, once brought to life, takes one of the four normal-priority hardware queues for the rest of the process -- four env handles then
    // share three (measured in round 6's first bench refresh: 3.6 -> 2.5 G env.step/s with four handles; docs/history.md section 5 has the mechanism)
    S.evtab = num_players <= 10 ? eval7_table(device, h->stream) : nullptr;

    // Game.__init__ (game.py:242-264): every seat ACTIVE, dealer cursor = config dealer, credits 0, ranks NONE.
    {
        std::vector<uint64_t> ss(T, (uint64_t)((1u << num_players) - 1));
        int d = ((dealer % num_players) + num_players) % num_players;
        std::vector<uint32_t> cur(T, (uint32_t)d << 4);
        std::vector<uint32_t> show(N * T, NONE_V);
        // get_valid_actions on the un-reset state (all credits and pending bets 0): raises invalid (0 > 0 is false),
        // CHECK valid (high_bet == 0), CALL invalid (0 < 0 is false) -> FOLD | CHECK | ALL_IN
        std::vector<uint8_t> valid(T, (uint8_t)((1u << MV_FOLD) | (1u << MV_CHECK) | (1u << MV_ALL_IN)));
        h->hot.fresh = d_fresh;
        h->hot.big_blind = big_blind; h->hot.small_blind = small_blind; h->hot.start_credits = d_start; h->hot.show = S.show;
        h->hot.key0 = S.key0; h->hot.key1 = S.key1; h->hot.table_id_base = table_id_base; h->hot.T = num_tables; h->hot.tpb = h->tpb; h->hot.prof = S.prof;
        h->hot.start_uniform = S.start_credits[0]; h->hot.start_is_uniform = 1;
        for (int i = 1; i < num_players; ++i) if (S.start_credits[i] != S.start_credits[0]) h->hot.start_is_uniform = 0;
        h->hot_env = h->hot; h->hot_env.tpb = h->env_tpb;
        if (hipMemcpyAsync(d_start, S.start_credits, PK_MAX_PLAYERS * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
            hipMemcpyAsync(h->d_S, &h->S, sizeof(State), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
            hipMemcpyAsync(S.seat_states, ss.data(), T * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
            hipMemcpyAsync(S.cursors, cur.data(), T * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
            hipMemcpyAsync(S.show, show.data(), N * T * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
            hipMemcpyAsync(S.valid, valid.data(), T, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess)
            return bail(h->fail(PK_E_HIP, "initial state upload"));
        if (seat_launch(h, SEAT_KERNEL(k_make_fresh, 1, h->stream, h->hot, d_fresh)) || hipStreamSynchronize(h->stream) != hipSuccess)
            return bail(h->fail(PK_E_HIP, "k_make_fresh"));
    }
    *out = h;
    return PK_OK;
}

int pk_destroy(pk_handle *h) {
    if (!h) return PK_OK;
    DeviceGuard guard(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->arena) (void)hipFree(h->arena);
    h->d_obs_packed.drop();
    if (h->snap_word) (void)hipFree(h->snap_word);
    if (h->snap_mark) (void)hipFree(h->snap_mark);
    h->snap_stage.drop();
    if (h->snap_ev) (void)hipEventDestroy(h->snap_ev);
    if (h->h_pinned) (void)hipHostFree(h->h_pinned);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    for (int i = 0; i < 2; ++i) if (h->ev_ring[i]) (void)hipEventDestroy(h->ev_ring[i]);
    for (int b = 0; b < PK_MAX_ENV_BATCHES; ++b) {
        stream_release(h->device, h->env_streams[b], true);
        if (h->env_done[b]) (void)hipEventDestroy(h->env_done[b]);
    }
    if (h->env_in) (void)hipEventDestroy(h->env_in);
    stream_release(h->device, h->own_stream);
    delete h;
    return PK_OK;
}

int pk_stream_pool_drain(int device) {
    if (device < -1 || device >= PK_MAX_DEVICES) { g_err = "pk_stream_pool_drain: device index out of range (-1 = every device)"; return PK_E_INVALID_ARG; }
    return drain_stream_pool(device);
}

int pk_num_tables(const pk_handle *h) { return h ? h->T : PK_E_INVALID_ARG; }
int pk_num_players(const pk_handle *h) { return h ? h->N : PK_E_INVALID_ARG; }
int pk_get_wave_shape(pk_handle *h, int *tables_per_wave, int *env_tables_per_wave) {
    if (!h || !tables_per_wave || !env_tables_per_wave) return h ? h->fail(PK_E_INVALID_ARG, "pk_get_wave_shape: NULL argument") : PK_E_INVALID_ARG;
    *tables_per_wave = h->tpb; *env_tables_per_wave = h->env_tpb;
    return PK_OK;
}

// ---- stream control: how a caller with its own stream (a learner on the same GPU) orders its work against ours
int pk_get_stream(pk_handle *h, void **stream_out) {
    if (!h || !stream_out) return PK_E_INVALID_ARG;
    *stream_out = (void *)h->stream;
    return PK_OK;
}
static int switch_stream(pk_handle *h, hipStream_t to) {
    if (!in_flight(h)) FLUSH(h);                 // host-side accumulated / deferred rollout steps belong to the old stream
    HIPCHK(h, hipStreamSynchronize(h->stream));  // nothing of ours may still be running on the stream we leave
    h->stream = to;
    h->ev_used[0] = h->ev_used[1] = false;
    return PK_OK;
}
int pk_set_stream(pk_handle *h, void *stream) {
    if (!h) return PK_E_INVALID_ARG;
    ON_DEVICE(h);
    if (stream) {   // a stream of another device would make every later launch fail (or, worse, run there)
        hipDevice_t dev = -1;
        if (hipStreamGetDevice((hipStream_t)stream, &dev) != hipSuccess) { (void)hipGetLastError(); return h->fail(PK_E_INVALID_ARG, "pk_set_stream: not a valid hipStream_t"); }
        if ((int)dev != h->device) return h->fail(PK_E_INVALID_ARG, "pk_set_stream: the stream belongs to another device than the handle");
    }
    return switch_stream(h, (hipStream_t)stream);   // NULL = the legacy default stream (what torch's default stream is)
}
int pk_use_own_stream(pk_handle *h) {
    if (!h) return PK_E_INVALID_ARG;
    ON_DEVICE(h);
    return switch_stream(h, h->own_stream);
}
int pk_wait_event(pk_handle *h, void *event) {
    if (!h || !event) return PK_E_INVALID_ARG;
    ON_DEVICE(h);
    // rollout steps the host still holds back (coalescing) were requested BEFORE this wait: launch them now, so that they do not
    // queue up behind the caller's event (and overlap with whatever the caller does until it records it)
    if (!in_flight(h) && h->acc > 0) { int rc = launch_coalesced(h, h->pend_policy, h->pend_auto); if (rc) return rc; }
    HIPCHK(h, hipStreamWaitEvent(h->stream, (hipEvent_t)event, 0));
    return PK_OK;
}
int pk_record_event(pk_handle *h, void *event) {
    if (!h || !event) return PK_E_INVALID_ARG;
    ON_DEVICE(h);
    if (!in_flight(h)) FLUSH(h);    // "everything requested so far" includes deferred rollout steps (env steps in flight stay so)
    // ... and the launches of pk_env_step_async_d's sub-batches on the handle's internal streams (pk_set_env_batches)
    for (int b = 0; b < h->env_batches && h->env_batches > 1; ++b)
        if (h->env_launched[b]) HIPCHK(h, hipStreamWaitEvent(h->stream, h->env_done[b], 0));
    HIPCHK(h, hipEventRecord((hipEvent_t)event, h->stream));
    return PK_OK;
}

int pk_set_tuning(pk_handle *h, int park, int endk) {
    if (!h) return PK_E_INVALID_ARG;
    if (park >= 1 && park <= 64) h->park = park;
    if (endk >= 1 && endk <= 64) h->endk = endk;
    return PK_OK;
}

static int upload_mask(pk_handle *h, const uint8_t *mask, const uint8_t **dmask) {
    *dmask = nullptr;
    if (mask) {
        HIPCHK(h, hipMemcpyAsync(h->d_mask, mask, (size_t)h->T, hipMemcpyHostToDevice, h->stream));
        *dmask = h->d_mask;
    }
    return PK_OK;
}

int pk_reset(pk_handle *h, const uint8_t *mask, int dealer) {
    if (!h) return PK_E_INVALID_ARG;
    ON_DEVICE(h);
    FLUSH(h);
    const uint8_t *dmask;
    int rc = upload_mask(h, mask, &dmask);
    if (rc) return rc;
    int d = ((dealer % h->N) + h->N) % h->N;
    if ((rc = seat_launch(h, SEAT_KERNEL(k_reset, table_grid(h), h->stream, h->S, h->hot, dmask, 0xff, d)))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PK_OK;
}

int pk_reset_d(pk_handle *h, const uint8_t *mask_d, int mask_bits, int dealer) {
    if (!h) return PK_E_INVALID_ARG;
    if (mask_d && !(mask_bits & 0xff)) return h->fail(PK_E_INVALID_ARG, "pk_reset_d: mask_bits selects no bit of a mask byte");
    ON_DEVICE(h);
    FLUSH(h);
    int d = ((dealer % h->N) + h->N) % h->N;
    return seat_launch(h, SEAT_KERNEL(k_reset, table_grid(h), h->stream, h->S, h->hot, mask_d, mask_bits & 0xff, d));
}

static int launch_step(pk_handle *h, const int32_t *actions_d, uint8_t *flags_d, uint8_t *terr_d, int auto_reset) {
    ON_DEVICE(h);
    FLUSH(h);
    const StepKernArgs ka{(const State *)h->d_S, h->hot, actions_d, flags_d, terr_d, scaled_park(h, 28), auto_reset ? 1 : 0, nullptr, 0, h->step_obs, h->step_obs_packed};
    return seat_launch(h, SEAT_KERNEL(k_step, table_grid(h), h->stream, ka));
}
int pk_step_d(pk_handle *h, const int32_t *actions_d, uint8_t *flags_d, uint8_t *terr_d) {
    if (!h || !actions_d || !flags_d) return h ? h->fail(PK_E_INVALID_ARG, "pk_step_d: NULL buffer") : PK_E_INVALID_ARG;
    return launch_step(h, actions_d, flags_d, terr_d, 0);
}
int pk_step_auto_d(pk_handle *h, const int32_t *actions_d, uint8_t *flags_d, uint8_t *terr_d) {
    if (!h || !actions_d || !flags_d) return h ? h->fail(PK_E_INVALID_ARG, "pk_step_auto_d: NULL buffer") : PK_E_INVALID_ARG;
    return launch_step(h, actions_d, flags_d, terr_d, 1);
}
int pk_step_async_d(pk_handle *h, const int32_t *actions_d, uint8_t *flags_d, uint8_t *terr_d, uint8_t *ready_d, int max_hands, int auto_reset) {
    if (!h || !flags_d || !ready_d) return h ? h->fail(PK_E_INVALID_ARG, "pk_step_async_d: NULL buffer") : PK_E_INVALID_ARG;
    if (!actions_d && max_hands > 0) return h->fail(PK_E_INVALID_ARG, "pk_step_async_d: actions_d may be NULL only for a drain (max_hands <= 0): finish what is in flight, step nothing");
    ON_DEVICE(h);
    if (h->step_pending) {
        if ((auto_reset ? 1 : 0) != h->step_auto)   // steps in flight keep the reset rule they were started with
            return h->fail(PK_E_INVALID_ARG, "pk_step_async_d: Game.steps are in flight with another auto_reset; drain them first (max_hands = 0)");
        if (h->env_pending || h->host_step) return flush(h);
    } else FLUSH(h);
    const StepKernArgs ka{(const State *)h->d_S, h->hot, actions_d, flags_d, terr_d, scaled_park(h, 28), auto_reset ? 1 : 0, ready_d, max_hands > 0 ? max_hands : 0,
                          h->step_obs, h->step_obs_packed};
    if (int rc = seat_launch(h, SEAT_KERNEL(k_step_async, table_grid(h), h->stream, ka))) return rc;
    h->step_pending = max_hands > 0;
    h->step_auto = auto_reset ? 1 : 0;
    return PK_OK;
}

static int any_terr(const uint8_t *terr, int T) {
    for (int i = 0; i < T; ++i) if (terr[i]) return 1;
    return 0;
}

int pk_step(pk_handle *h, const int32_t *actions, uint8_t *flags, uint8_t *terr) {
    if (!h || !actions || !flags) return h ? h->fail(PK_E_INVALID_ARG, "pk_step: NULL buffer") : PK_E_INVALID_ARG;
    ON_DEVICE(h);
    if (in_flight(h)) return flush(h);     // PK_E_BUSY, before anything is queued
    const size_t T = (size_t)h->T;
    HIPCHK(h, hipMemcpyAsync(h->d_actions, actions, T * 4, hipMemcpyHostToDevice, h->stream));
    int rc = pk_step_d(h, h->d_actions, h->d_flags, h->d_terr);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(flags, h->d_flags, T, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->h_pinned, h->d_terr, T, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (terr) memcpy(terr, h->h_pinned, T);
    if (any_terr(h->h_pinned, h->T)) return h->fail(PK_E_TABLE, "pk_step: per-table error(s), see terr");
    return PK_OK;
}

static int bad_player(const pk_handle *h, int player) { return player >= h->N; }

// The launches of the getters that have a host form (export_to_host into h->d_export) and a device form (FLUSH_READER, the caller's buffer)
static void launch_valid_actions(pk_handle *h, int player, uint8_t *out) {
    hipLaunchKernelGGL(k_export_valid, dim3(flat_grid((size_t)h->T * PK_NUM_MOVES)), dim3(256), 0, h->stream, h->S, h->N, player, out);
}
static void launch_f64(pk_handle *h, int field, double *out) {
    const double *src = field == PK_F_CREDITS ? h->S.credits : field == PK_F_BETS ? h->S.bets : field == PK_F_PENDING_BETS ? h->S.pending : h->S.payoffs;
    hipLaunchKernelGGL(k_export_f64, dim3(flat_grid((size_t)h->T * h->N)), dim3(256), 0, h->stream, src, h->T, h->N, out);
}
static void launch_obs(pk_handle *h, int player, double *out) {
    hipLaunchKernelGGL(k_obs, dim3(obs_grid(h->T)), dim3(OBS_BLOCK), 0, h->stream, h->S, h->N, player, out);
}
static void launch_obs_packed(pk_handle *h, int player, uint8_t *out) {
    hipLaunchKernelGGL(k_obs_packed, dim3(obs_grid(h->T)), dim3(OBS_BLOCK), 0, h->stream, h->S, h->N, player, out);
}

int pk_get_valid_actions(pk_handle *h, int player, uint8_t *out) {
    if (!h || !out || bad_player(h, player)) return h ? h->fail(PK_E_INVALID_ARG, "pk_get_valid_actions: bad argument") : PK_E_INVALID_ARG;
    return export_to_host(h, out, (size_t)h->T * PK_NUM_MOVES, [&] { launch_valid_actions(h, player, (uint8_t *)h->d_export); });
}

int pk_get_f64(pk_handle *h, int field, double *out) {
    if (!h || !out || field < 0 || field > 3) return h ? h->fail(PK_E_INVALID_ARG, "pk_get_f64: bad field") : PK_E_INVALID_ARG;
    return export_to_host(h, out, (size_t)h->T * h->N * 8, [&] { launch_f64(h, field, (double *)h->d_export); });
}

int pk_get_f64_d(pk_handle *h, int field, double *out_d) {
    if (!h || !out_d || field < 0 || field > 3) return h ? h->fail(PK_E_INVALID_ARG, "pk_get_f64_d: bad argument") : PK_E_INVALID_ARG;
    ON_DEVICE(h);
    FLUSH_READER(h);
    launch_f64(h, field, out_d);
    HIPCHK(h, hipGetLastError());
    return PK_OK;
}

int pk_get_table_f64(pk_handle *h, int field, double *out) {
    if (!h || !out || field < 0 || field > PK_TF_MIN_RAISE) return h ? h->fail(PK_E_INVALID_ARG, "pk_get_table_f64: bad field") : PK_E_INVALID_ARG;
    return export_to_host(h, out, (size_t)h->T * 8, [&] {
        hipLaunchKernelGGL(k_table_f64, dim3(flat_grid(h->T)), dim3(256), 0, h->stream, h->S, h->N, field, (double *)h->d_export);
    });
}

int pk_get_min_raise(pk_handle *h, double *out) { return pk_get_table_f64(h, PK_TF_MIN_RAISE, out); }

int pk_get_game_over(pk_handle *h, uint8_t *out) {
    if (!h || !out) return PK_E_INVALID_ARG;
    return export_to_host(h, out, (size_t)h->T, [&] {
        hipLaunchKernelGGL(k_game_over, dim3(flat_grid(h->T)), dim3(256), 0, h->stream, h->S.seat_states, h->T, h->N, (uint8_t *)h->d_export);
    });
}

int pk_get_player_states(pk_handle *h, uint8_t *out) {
    if (!h || !out) return PK_E_INVALID_ARG;
    size_t n = (size_t)h->T * h->N;
    return export_to_host(h, out, n, [&] {
        hipLaunchKernelGGL(k_export_states, dim3(flat_grid(n)), dim3(256), 0, h->stream, h->S.seat_states, h->T, h->N, (uint8_t *)h->d_export);
    });
}

int pk_get_i32(pk_handle *h, int field, int32_t *out) {
    if (!h || !out || field < 0 || field > PK_I_HAND) return h ? h->fail(PK_E_INVALID_ARG, "pk_get_i32: bad field") : PK_E_INVALID_ARG;
    return export_to_host(h, out, (size_t)h->T * 4, [&] {
        hipLaunchKernelGGL(k_export_i32, dim3(flat_grid(h->T)), dim3(256), 0, h->stream, h->S, field, (int32_t *)h->d_export);
    });
}

int pk_get_serials(pk_handle *h, uint64_t *hand_serial, uint64_t *step_serial) {
    if (!h) return PK_E_INVALID_ARG;
    ON_DEVICE(h);
    if (!h->env_pending) FLUSH(h);   // with env steps in flight: the counts of the hands dealt / Game.steps completed so far
    if (hand_serial) HIPCHK(h, hipMemcpyAsync(hand_serial, h->S.hand_serial, (size_t)h->T * 8, hipMemcpyDeviceToHost, h->stream));
    if (step_serial) HIPCHK(h, hipMemcpyAsync(step_serial, h->S.step_serial, (size_t)h->T * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PK_OK;
}

int pk_set_serials(pk_handle *h, const uint64_t *hand_serial, const uint64_t *step_serial) {
    if (!h) return PK_E_INVALID_ARG;
    ON_DEVICE(h);
    FLUSH(h);
    if (hand_serial) HIPCHK(h, hipMemcpyAsync(h->S.hand_serial, hand_serial, (size_t)h->T * 8, hipMemcpyHostToDevice, h->stream));
    if (step_serial) HIPCHK(h, hipMemcpyAsync(h->S.step_serial, step_serial, (size_t)h->T * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PK_OK;
}

int pk_get_cards(pk_handle *h, uint8_t *out) {
    if (!h || !out) return PK_E_INVALID_ARG;
    int K = 5 + 2 * h->N;
    size_t n = (size_t)h->T * K;
    return export_to_host(h, out, n, [&] {
        hipLaunchKernelGGL(k_export_cards, dim3(flat_grid(n)), dim3(256), 0, h->stream, h->S.cards, h->T, K, (uint8_t *)h->d_export);
    });
}

int pk_get_hand_ranks(pk_handle *h, uint8_t *rank, uint32_t *kick) {
    if (!h || !rank || !kick) return PK_E_INVALID_ARG;
    ON_DEVICE(h);
    FLUSH(h);
    size_t n = (size_t)h->T * h->N;
    uint32_t *dk = (uint32_t *)h->d_export;
    uint8_t *dr = (uint8_t *)h->d_export + n * 4;
    if (n * 5 > h->export_bytes) return h->fail(PK_E_INVALID_ARG, "export buffer too small");
    hipLaunchKernelGGL(k_export_show, dim3(flat_grid(n)), dim3(256), 0, h->stream, h->S.show, h->T, h->N, dr, dk);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(kick, dk, n * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(rank, dr, n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PK_OK;
}

int pk_get_obs(pk_handle *h, int player, double *out) {
    if (!h || !out || bad_player(h, player)) return h ? h->fail(PK_E_INVALID_ARG, "pk_get_obs: bad argument") : PK_E_INVALID_ARG;
    return export_to_host(h, out, (size_t)h->T * PK_OBS_DIM(h->N) * 8, [&] { launch_obs(h, player, (double *)h->d_export); });
}

int pk_get_obs_d(pk_handle *h, int player, double *out_d) {
    if (!h || !out_d || bad_player(h, player)) return h ? h->fail(PK_E_INVALID_ARG, "pk_get_obs_d: bad argument") : PK_E_INVALID_ARG;
    ON_DEVICE(h);
    FLUSH_READER(h);
    launch_obs(h, player, out_d);
    HIPCHK(h, hipGetLastError());
    return PK_OK;
}

int pk_get_obs_packed(pk_handle *h, int player, uint8_t *out) {
    if (!h || !out || bad_player(h, player)) return h ? h->fail(PK_E_INVALID_ARG, "pk_get_obs_packed: bad argument") : PK_E_INVALID_ARG;
    return export_to_host(h, out, (size_t)h->T * PK_OBS_PACKED_BYTES(h->N), [&] { launch_obs_packed(h, player, (uint8_t *)h->d_export); });
}

int pk_get_obs_packed_d(pk_handle *h, int player, uint8_t *out_d) {
    if (!h || !out_d || bad_player(h, player) || ((uintptr_t)out_d & 7)) return h ? h->fail(PK_E_INVALID_ARG, "pk_get_obs_packed_d: bad argument (out_d must be 8-byte aligned)") : PK_E_INVALID_ARG;
    ON_DEVICE(h);
    FLUSH_READER(h);
    launch_obs_packed(h, player, out_d);
    HIPCHK(h, hipGetLastError());
    return PK_OK;
}

int pk_set_env_obs_packed(pk_handle *h, uint8_t *obs_packed_d) {
    if (!h || ((uintptr_t)obs_packed_d & 7)) return h ? h->fail(PK_E_INVALID_ARG, "pk_set_env_obs_packed: the buffer must be 8-byte aligned") : PK_E_INVALID_ARG;
    if (in_flight(h)) return h->fail(PK_E_BUSY, "pk_set_env_obs_packed: PokerGameEnv steps are in flight");
    h->env_obs_packed = obs_packed_d;
    return PK_OK;
}

int pk_set_step_obs(pk_handle *h, double *obs_d, uint8_t *obs_packed_d) {
    if (!h || ((uintptr_t)obs_d & 7) || ((uintptr_t)obs_packed_d & 7)) return h ? h->fail(PK_E_INVALID_ARG, "pk_set_step_obs: the buffers must be 8-byte aligned") : PK_E_INVALID_ARG;
    if (in_flight(h)) return h->fail(PK_E_BUSY, "pk_set_step_obs: steps are in flight; drain them first");
    h->step_obs = obs_d; h->step_obs_packed = obs_packed_d;
    return PK_OK;
}

int pk_host_alloc(void **out, size_t bytes) {
    if (!out || bytes == 0) { g_err = "pk_host_alloc: bad argument"; return PK_E_INVALID_ARG; }
    *out = nullptr;
    if (int rc = check_device("pk_host_alloc", 0)) return rc;
    hipError_t e = hipHostMalloc(out, bytes, hipHostMallocPortable);
    if (e != hipSuccess) { *out = nullptr; return g_fail(PK_E_OOM, "pk_host_alloc", e); }
    return PK_OK;
}

int pk_host_free(void *p) {
    if (!p) return PK_OK;
    return hipHostFree(p) == hipSuccess ? PK_OK : PK_E_HIP;
}

// Game.step's precondition (game.py:648-651) for a whole batch WITHOUT touching a table: index of the first table whose
// action is not valid for its active player, or -1.
int pk_check_actions(pk_handle *h, const int32_t *actions, int32_t *first_bad) {
    if (!h || !actions || !first_bad) return h ? h->fail(PK_E_INVALID_ARG, "pk_check_actions: NULL buffer") : PK_E_INVALID_ARG;
    ON_DEVICE(h);
    FLUSH(h);
    const size_t T = (size_t)h->T;
    int32_t *slot = (int32_t *)h->d_totals;                         // (8-byte slot 0 of the counters' output: free between calls)
    const int32_t init = 0x7fffffff;
    HIPCHK(h, hipMemcpyAsync(h->d_actions, actions, T * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(slot, &init, 4, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_check_actions, dim3(flat_grid(T)), dim3(256), 0, h->stream, h->S.valid, h->d_actions, h->T, slot);
    HIPCHK(h, hipGetLastError());
    int32_t got = 0;
    HIPCHK(h, hipMemcpyAsync(&got, slot, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *first_bad = got == init ? -1 : got;
    return PK_OK;
}

int pk_get_valid_actions_d(pk_handle *h, int player, uint8_t *out_d) {
    if (!h || !out_d || bad_player(h, player)) return h ? h->fail(PK_E_INVALID_ARG, "pk_get_valid_actions_d: bad argument") : PK_E_INVALID_ARG;
    ON_DEVICE(h);
    FLUSH_READER(h);
    launch_valid_actions(h, player, out_d);
    HIPCHK(h, hipGetLastError());
    return PK_OK;
}

int pk_env_reset_d(pk_handle *h, const uint8_t *mask_d, int opp_policy) {
    if (!h || bad_policy(opp_policy)) return h ? h->fail(PK_E_INVALID_ARG, "pk_env_reset_d: bad argument") : PK_E_INVALID_ARG;
    ON_DEVICE(h);
    FLUSH(h);
    const EnvResetKernArgs ka{(const State *)h->d_S, h->hot_env, mask_d, uniform_seats(opp_policy), env_park(h)};
    return seat_launch(h, SEAT_KERNEL(k_env_reset, env_grid(h), h->stream, ka));
}

int pk_env_step_d(pk_handle *h, const int32_t *actions_d, int opp_policy, double *reward_d, uint8_t *done_d,
                  uint8_t *hand_d, uint8_t *terr_d) {
    if (!h || !actions_d || !reward_d || !done_d || !hand_d || !terr_d || bad_policy(opp_policy))
        return h ? h->fail(PK_E_INVALID_ARG, "pk_env_step_d: bad argument") : PK_E_INVALID_ARG;
    ON_DEVICE(h);
    FLUSH(h);
    const EnvKernArgs ka = env_args(h, actions_d, -1, uniform_seats(opp_policy), 0, reward_d, done_d, hand_d, terr_d, nullptr);
    return seat_launch(h, SEAT_KERNEL(k_env_step, env_grid(h), h->stream, ka));
}

int pk_env_step_fused_d(pk_handle *h, const int32_t *actions_d, int seat0_policy, int opp_policy, int auto_reset,
                        double *reward_d, uint8_t *done_d, uint8_t *hand_d, uint8_t *terr_d, double *obs_d) {
    if (!h || !reward_d || !done_d || !hand_d || !terr_d || bad_policy(opp_policy) ||
        (!actions_d && (bad_policy(seat0_policy))))
        return h ? h->fail(PK_E_INVALID_ARG, "pk_env_step_fused_d: bad argument") : PK_E_INVALID_ARG;
    ON_DEVICE(h);
    FLUSH(h);
    const EnvKernArgs ka = with_packed(h, env_args(h, actions_d, actions_d ? -1 : seat0_policy, uniform_seats(opp_policy), auto_reset ? 1 : 0, reward_d, done_d, hand_d, terr_d, obs_d));
    return seat_launch(h, SEAT_KERNEL(k_env_step, env_grid(h), h->stream, ka));
}

int pk_env_step_async_d(pk_handle *h, const int32_t *actions_d, int seat0_policy, int opp_policy, int auto_reset, int max_passes,
                        double *reward_d, uint8_t *done_d, uint8_t *hand_d, uint8_t *terr_d, double *obs_d, uint8_t *ready_d) {
    if (!h || !reward_d || !done_d || !hand_d || !terr_d || !ready_d || bad_policy(opp_policy) ||
        (!actions_d && (bad_policy(seat0_policy))))
        return h ? h->fail(PK_E_INVALID_ARG, "pk_env_step_async_d: bad argument") : PK_E_INVALID_ARG;
    ON_DEVICE(h);
    if (h->host_step || h->step_pending) return flush(h);   // PK_E_BUSY: a host-buffer step awaits its end / Game.steps are in flight
    const int s0 = actions_d ? -1 : seat0_policy, au = auto_reset ? 1 : 0;
    // steps in flight keep THEIR agents and reset rule (as owed rollout steps do): a call that would change them is refused
    if (h->env_pending && (h->env_multi || s0 != h->env_seat0 || opp_policy != h->env_opp || au != h->env_auto))
        return h->fail(PK_E_INVALID_ARG, "pk_env_step_async_d: seat-0 source, opp_policy and auto_reset must stay the same while steps are in flight (drain with max_passes = 0 first)");
    h->env_seat0 = s0; h->env_opp = opp_policy; h->env_auto = au;
    int rc = flush_rollout(h);
    if (rc) return rc;
    const int mp = max_passes > 0 ? max_passes : 0;
    if (h->env_batches <= 1) {
        EnvKernArgs ka = with_packed(h, env_args(h, actions_d, actions_d ? -1 : seat0_policy, uniform_seats(opp_policy), au, reward_d, done_d, hand_d, terr_d, obs_d));
        ka.A.ready = ready_d; ka.A.max_passes = mp;
        if ((rc = seat_launch(h, SEAT_KERNEL(k_env_step_async, env_grid(h), h->stream, ka)))) return rc;
        h->env_last_begin = 0; h->env_last_end = h->T; h->env_last_fresh = 0;
    } else {
        // the caller's writes so far (actions of the range about to be launched) order before the launch(es) below
        // ... unless that stream is IDLE (everything the caller queued there has completed: a host-side learner, bench.py): then
        // there is nothing to order, and no barrier packet is put into any queue (see the note on the delivery wait below)
        hipError_t qs = hipStreamQuery(h->stream);
        if (qs != hipSuccess && qs != hipErrorNotReady) return h->fail(PK_E_HIP, "hipStreamQuery", qs);
        if (qs == hipErrorNotReady) (void)hipGetLastError();
        const bool caller_busy = qs == hipErrorNotReady;
        if (caller_busy) HIPCHK(h, hipEventRecord(h->env_in, h->stream));
        auto launch_range = [&](int b, int passes) -> int {
            const int t0 = b * h->env_range, tend = (t0 + h->env_range < h->T) ? t0 + h->env_range : h->T;
            if (caller_busy) HIPCHK(h, hipStreamWaitEvent(h->env_streams[b], h->env_in, 0));
            EnvKernArgs ka = with_packed(h, env_args(h, actions_d, actions_d ? -1 : seat0_policy, uniform_seats(opp_policy), au, reward_d, done_d, hand_d, terr_d, obs_d));
            ka.A.ready = ready_d; ka.A.max_passes = passes; ka.A.t0 = t0; ka.A.tend = tend;
            if (int rc_ = seat_launch(h, SEAT_KERNEL(k_env_step_async, (tend - t0 + h->env_tpb - 1) / h->env_tpb, h->env_streams[b], ka))) return rc_;
            HIPCHK(h, hipEventRecord(h->env_done[b], h->env_streams[b]));
            return PK_OK;
        };
        if (mp == 0) {   // drain: every range runs to its end; everything is delivered
            for (int b = 0; b < h->env_batches; ++b) { rc = launch_range(b, 0); if (rc) return rc; }
            for (int b = 0; b < h->env_batches; ++b) { HIPCHK(h, hipStreamWaitEvent(h->stream, h->env_done[b], 0)); h->env_launched[b] = false; }
            // everything is delivered; the next bounded call starts the round again with range 0
            h->env_last_begin = 0; h->env_last_end = h->T; h->env_last_fresh = 0; h->env_next = 0;
        } else {         // launch one range, deliver the one launched longest ago (the next in the round)
            const int b = h->env_next, d = (b + 1) % h->env_batches;
            rc = launch_range(b, mp);
            if (rc) return rc;
            h->env_launched[b] = true;
            h->env_last_fresh = h->env_launched[d] ? 0 : 1;
            // Delivery of the range launched longest ago.  The HOST waits for it (it was launched B - 1 calls ago and is done or
            // nearly so), then the caller's stream needs no device-side dependency at all.  A hipStreamWaitEvent on the caller's
            // stream is a barrier packet parked at the head of its hardware queue: when that queue happens to share a pipe of the
            // command processor with one of the range queues (which queues share depends on how many the process created before),
            // the parked barrier holds that range's dispatches back -- the same call sequence ran at 1.5 G env.step/s in a process
            // that had used another PokerGameEnv handle before, 3.6 G in a fresh one.
            if (h->env_launched[d]) HIPCHK(h, hipEventSynchronize(h->env_done[d]));
            h->env_last_begin = d * h->env_range;
            h->env_last_end = (h->env_last_begin + h->env_range < h->T) ? h->env_last_begin + h->env_range : h->T;
            h->env_next = d;
        }
    }
    h->env_pending = max_passes > 0;
    h->env_multi = false;
    return PK_OK;
}

int pk_set_env_batches(pk_handle *h, int batches) {
    if (!h || batches < 1 || batches > PK_MAX_ENV_BATCHES) return h ? h->fail(PK_E_INVALID_ARG, "pk_set_env_batches: 1 <= batches <= PK_MAX_ENV_BATCHES") : PK_E_INVALID_ARG;
    ON_DEVICE(h);
    FLUSH(h);                                         // PK_E_BUSY while env steps are in flight: drain first
    HIPCHK(h, hipStreamSynchronize(h->stream));
    int range = (h->T + batches - 1) / batches;
    range = (range + 63) / 64 * 64;                   // whole waves per range
    const int nb = (h->T + range - 1) / range;        // (fewer ranges than asked for when the batch is small)
    for (int b = 0; b < nb && nb > 1; ++b) {
        if (!h->env_streams[b]) HIPCHK(h, stream_acquire(h->device, &h->env_streams[b], true));
        if (!h->env_done[b]) HIPCHK(h, hipEventCreateWithFlags(&h->env_done[b], hipEventDisableTiming));
        h->env_launched[b] = false;
    }
    if (nb > 1 && !h->env_in) HIPCHK(h, hipEventCreateWithFlags(&h->env_in, hipEventDisableTiming));
    h->env_batches = nb; h->env_range = range; h->env_next = 0;
    // "the range one call delivers is the range the next call launches": before the first call that is range 0, untouched
    h->env_last_begin = 0; h->env_last_end = nb > 1 ? (range < h->T ? range : h->T) : h->T; h->env_last_fresh = nb > 1 ? 1 : 0;
    return PK_OK;
}

int pk_env_last_range(pk_handle *h, int *begin, int *end, int *fresh) {
    if (!h) return PK_E_INVALID_ARG;
    if (begin) *begin = h->env_last_begin;
    if (end) *end = h->env_last_end;
    if (fresh) *fresh = h->env_last_fresh;
    return PK_OK;
}

static int check_seat_policies(pk_handle *h, uint64_t seat_policies, bool *any_external) {
    *any_external = false;
    for (int p = 0; p < h->N; ++p) {
        const int pol = PK_SEAT_POLICY(seat_policies, p);
        if (pol == PK_POLICY_EXTERNAL) *any_external = true;
        else if (bad_policy(pol)) return h->fail(PK_E_INVALID_ARG, "seat_policies: nibble p must be PK_POLICY_RANDOM / _ALLIN / _CALL or PK_POLICY_EXTERNAL for every seat p < num_players");
    }
    return PK_OK;
}

int pk_env_step_multi_d(pk_handle *h, const int32_t *actions_d, const uint8_t *reset_d, uint64_t seat_policies, int auto_reset,
                        int max_passes, double *reward_d, uint8_t *done_d, uint8_t *hand_d, uint8_t *terr_d, double *obs_d,
                        uint8_t *who_d, uint8_t *ready_d) {
    if (!h || !reward_d || !done_d || !hand_d || !terr_d || !ready_d || !who_d)
        return h ? h->fail(PK_E_INVALID_ARG, "pk_env_step_multi_d: NULL buffer") : PK_E_INVALID_ARG;
    bool ext = false;
    int rc = check_seat_policies(h, seat_policies, &ext);
    if (rc) return rc;
    if (ext && !actions_d) return h->fail(PK_E_INVALID_ARG, "pk_env_step_multi_d: actions_d is required when a seat is PK_POLICY_EXTERNAL");
    ON_DEVICE(h);
    if (h->host_step || h->step_pending) return flush(h);   // PK_E_BUSY
    const int au = auto_reset ? 1 : 0;
    // steps in flight keep THEIR agents and reset rule: a call that would change them is refused
    if (h->env_pending && (!h->env_multi || seat_policies != h->env_seats || au != h->env_auto))
        return h->fail(PK_E_INVALID_ARG, "pk_env_step_multi_d: seat_policies and auto_reset must stay the same while steps are in flight (pk_env_end_multi_d first)");
    rc = flush_rollout(h);
    if (rc) return rc;
    const int pol0 = PK_SEAT_POLICY(seat_policies, 0);
    EnvKernArgs ka = with_packed(h, env_args(h, actions_d, pol0 == PK_POLICY_EXTERNAL ? -1 : pol0, seat_policies, au, reward_d, done_d, hand_d, terr_d, obs_d));
    ka.A.ready = ready_d; ka.A.max_passes = max_passes > 0 ? max_passes : 0; ka.A.reset_req = reset_d; ka.A.who = who_d;
    if ((rc = seat_launch(h, SEAT_KERNEL(k_env_step_multi, env_grid(h), h->stream, ka)))) return rc;
    // a table may be waiting for the caller's action for an external seat even after a drain: in flight until pk_env_end_multi_d
    h->env_pending = max_passes > 0 || ext;
    h->env_multi = true; h->env_seats = seat_policies; h->env_auto = au;
    return PK_OK;
}

int pk_env_end_multi_d(pk_handle *h) {
    if (!h) return PK_E_INVALID_ARG;
    ON_DEVICE(h);
    if (!h->env_pending) return PK_OK;
    if (!h->env_multi) return h->fail(PK_E_INVALID_ARG, "pk_env_end_multi_d: the steps in flight belong to pk_env_step_async_d (drain them with max_passes = 0)");
    const int pol0 = PK_SEAT_POLICY(h->env_seats, 0);
    // drain; what is still in flight afterwards waits for an external seat's action between two Game.steps and is abandoned.
    // Outputs of steps that return during this drain go to the handle's own staging buffers, i.e. are dropped.
    EnvKernArgs ka = env_args(h, nullptr, pol0 == PK_POLICY_EXTERNAL ? -1 : pol0, h->env_seats, h->env_auto, h->d_reward, h->d_done, h->d_handf, h->d_terr, nullptr);
    ka.A.ready = h->d_flags; ka.A.who = h->d_mask; ka.A.abandon = 1; ka.A.obs_packed = nullptr;
    if (int rc = seat_launch(h, SEAT_KERNEL(k_env_step_multi, env_grid(h), h->stream, ka))) return rc;
    h->env_pending = false; h->env_multi = false;
    return PK_OK;
}

int pk_pick_actions_d(pk_handle *h, int policy, int32_t *actions_d) {
    if (!h || !actions_d || bad_policy(policy)) return h ? h->fail(PK_E_INVALID_ARG, "pk_pick_actions_d: bad argument") : PK_E_INVALID_ARG;
    ON_DEVICE(h);
    FLUSH_READER(h);
    return seat_launch(h, SEAT_KERNEL(k_pick, table_grid(h), h->stream, h->S, h->hot, policy, actions_d));
}

int pk_pick_actions(pk_handle *h, int policy, int32_t *actions) {
    if (!h || !actions || bad_policy(policy)) return h ? h->fail(PK_E_INVALID_ARG, "pk_pick_actions: bad argument") : PK_E_INVALID_ARG;
    ON_DEVICE(h);
    int rc = pk_pick_actions_d(h, policy, h->d_actions);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(actions, h->d_actions, (size_t)h->T * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PK_OK;
}

static int fetch_counters(pk_handle *h, uint64_t *counters) {
    unsigned long long c[PK_NUM_COUNTERS];
    hipLaunchKernelGGL(k_sum_counters, dim3(1), dim3(256), 0, h->stream, h->S.counters, table_grid(h), h->d_totals);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(c, h->d_totals, sizeof(c), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < PK_NUM_COUNTERS; ++i) counters[i] += c[i];
    return PK_OK;
}

// fused: one launch that may leave work for later (counters == NULL) or must complete it (counters != NULL);
// unfused: k_steps complete single-step launches (state round-trips HBM every step).
static int enqueue_rollout(pk_handle *h, int k_steps, int policy, int auto_reset, int fused, bool complete, bool may_coalesce = true) {
    if (in_flight(h)) return flush(h);     // PK_E_BUSY (k_rollout would carry a Game.step of pk_step_async_d on as if it were deferred rollout work)
    if ((h->pending || h->acc) && (policy != h->pend_policy || auto_reset != h->pend_auto)) FLUSH(h);  // owed steps keep THEIR agents
    if (!fused) {
        FLUSH(h);
        for (int k = 0; k < k_steps; ++k) {
            int rc = launch_rollout(h, 1, policy, auto_reset, 1);
            if (rc) return rc;
        }
        return PK_OK;
    }
    if (k_steps == 0) return complete ? flush(h) : PK_OK;
    // deferral only in the throughput mode: without auto_reset a table that reports an error stops for the rest of THIS
    // call (and is retried by the next), so calls must not be merged
    if (complete || !auto_reset) {
        k_steps += h->acc; h->acc = 0;
        return launch_rollout(h, k_steps, policy, auto_reset, 1);
    }
    if (k_steps > (1 << 30) - h->acc) FLUSH(h);
    h->acc += k_steps;
    h->pend_policy = policy; h->pend_auto = auto_reset;
    if (may_coalesce && h->coalesce > 0 && h->acc < h->coalesce && h->ev_used[h->ev_idx]) {
        // the launch before the last one (the ring slot about to be reused) still running: two launches are in flight,
        // the GPU will not idle if this call just leaves its steps with the host
        hipError_t q = hipEventQuery(h->ev_ring[h->ev_idx]);
        if (q == hipErrorNotReady) { (void)hipGetLastError(); return PK_OK; }   // "not ready" is an answer, not an error to keep
        if (q != hipSuccess) return h->fail(PK_E_HIP, "hipEventQuery", q);
    }
    return launch_coalesced(h, policy, auto_reset);
}

int pk_rollout(pk_handle *h, int k_steps, int policy, int auto_reset, int fused, uint64_t *counters) {
    if (!h || k_steps < 0 || bad_policy(policy)) return h ? h->fail(PK_E_INVALID_ARG, "pk_rollout: bad argument") : PK_E_INVALID_ARG;
    ON_DEVICE(h);
    int rc = enqueue_rollout(h, k_steps, policy, auto_reset ? 1 : 0, fused, counters != nullptr);
    if (rc) return rc;
    if (counters) return fetch_counters(h, counters);
    return PK_OK;
}

int pk_set_coalesce(pk_handle *h, int max_steps) {
    if (!h || max_steps < 0 || max_steps > (1 << 20)) return h ? h->fail(PK_E_INVALID_ARG, "pk_set_coalesce: 0 <= max_steps <= 2^20") : PK_E_INVALID_ARG;
    h->coalesce = max_steps;
    return PK_OK;
}

int pk_get_launch_stats(pk_handle *h, uint64_t *out, int reset) {
    if (!h || !out) return PK_E_INVALID_ARG;
    out[0] = h->st_launches; out[1] = h->st_steps; out[2] = h->st_min; out[3] = h->st_max;
    if (reset) h->st_launches = h->st_steps = h->st_min = h->st_max = 0;
    return PK_OK;
}

int pk_get_owed(pk_handle *h, uint32_t *out) {
    if (!h || !out) return PK_E_INVALID_ARG;
    ON_DEVICE(h);
    HIPCHK(h, hipMemcpyAsync(out, h->S.owed, (size_t)h->T * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PK_OK;
}

int pk_flush(pk_handle *h) {
    if (!h) return PK_E_INVALID_ARG;
    ON_DEVICE(h);
    return flush(h);
}

int pk_time_rollout(pk_handle *h, int k_steps, int policy, int auto_reset, int fused, int reps, double *ms_per_launch,
                    uint64_t *counters) {
    if (!h || !ms_per_launch || reps < 1 || k_steps < 0 || bad_policy(policy))
        return h ? h->fail(PK_E_INVALID_ARG, "pk_time_rollout: bad argument") : PK_E_INVALID_ARG;
    ON_DEVICE(h);
    FLUSH(h);
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    for (int r = 0; r < reps; ++r) {
        // k_steps == 0: empty launches (load the tables, store them) -- the fixed cost of a launch, for diagnostics
        int rc = k_steps ? enqueue_rollout(h, k_steps, policy, auto_reset ? 1 : 0, fused, false, false)
                         : launch_rollout(h, 0, policy, auto_reset ? 1 : 0, 1);
        if (rc) return rc;
    }
    FLUSH(h);  // what the deferred launches left is part of the work that is being timed
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev1));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    int launches = reps * (fused ? 1 : k_steps);   // the flush is work of these launches: its time is shared among them
    *ms_per_launch = launches ? (double)ms / launches : 0.0;
    if (counters) return fetch_counters(h, counters);
    return PK_OK;
}

int pk_env_reset(pk_handle *h, const uint8_t *mask, int opp_policy) {
    if (!h || bad_policy(opp_policy)) return h ? h->fail(PK_E_INVALID_ARG, "pk_env_reset: bad argument") : PK_E_INVALID_ARG;
    ON_DEVICE(h);
    const uint8_t *dmask;
    int rc = upload_mask(h, mask, &dmask);
    if (rc) return rc;
    rc = pk_env_reset_d(h, dmask, opp_policy);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PK_OK;
}

int pk_env_step(pk_handle *h, const int32_t *actions, int opp_policy, double *reward, uint8_t *done, uint8_t *hand,
                uint8_t *terr) {
    if (!h || !actions || !reward || !done || !hand || bad_policy(opp_policy))
        return h ? h->fail(PK_E_INVALID_ARG, "pk_env_step: bad argument") : PK_E_INVALID_ARG;
    ON_DEVICE(h);
    if (in_flight(h)) return flush(h);     // PK_E_BUSY, before anything is queued
    const size_t T = (size_t)h->T;
    HIPCHK(h, hipMemcpyAsync(h->d_actions, actions, T * 4, hipMemcpyHostToDevice, h->stream));
    int rc = pk_env_step_d(h, h->d_actions, opp_policy, h->d_reward, h->d_done, h->d_handf, h->d_terr);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(reward, h->d_reward, T * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(done, h->d_done, T, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(hand, h->d_handf, T, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->h_pinned, h->d_terr, T, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (terr) memcpy(terr, h->h_pinned, T);
    if (any_terr(h->h_pinned, h->T)) return h->fail(PK_E_TABLE, "pk_env_step: per-table error(s), see terr");
    return PK_OK;
}

// PokerGameEnv.step through HOST buffers, in two halves: pk_env_step_begin uploads the actions, launches the step (seat 0 =
// the caller's actions; finished episodes reset on the spot when auto_reset != 0) and queues the copies of every output into
// the caller's buffers; pk_env_step_end waits for them.  With PINNED buffers (pk_host_alloc) nothing in `begin` blocks, the
// copies run at PCIe line rate, and the caller -- or another handle's step -- overlaps with them.  obs / obs_packed may be
// NULL (no row of that kind).  Between begin and end the handle may not be used otherwise.
int pk_env_step_begin(pk_handle *h, const int32_t *actions, int opp_policy, int auto_reset, double *reward, uint8_t *done,
                      uint8_t *hand, uint8_t *terr, double *obs, uint8_t *obs_packed) {
    if (!h || !actions || !reward || !done || !hand || !terr || bad_policy(opp_policy))
        return h ? h->fail(PK_E_INVALID_ARG, "pk_env_step_begin: bad argument") : PK_E_INVALID_ARG;
    ON_DEVICE(h);
    FLUSH(h);
    const size_t T = (size_t)h->T, D = (size_t)PK_OBS_DIM(h->N), PB = (size_t)PK_OBS_PACKED_BYTES(h->N);
    if (obs && T * D * 8 > h->export_bytes) return h->fail(PK_E_INVALID_ARG, "export buffer too small");
    uint8_t *d_packed = obs_packed ? (uint8_t *)h->d_obs_packed.reserve(T * PB, T * PB, h->stream) : nullptr;
    if (obs_packed && !d_packed) return h->fail(PK_E_HIP, "hipMalloc((void **)&h->d_obs_packed, T * PB)", h->d_obs_packed.err);
    HIPCHK(h, hipMemcpyAsync(h->d_actions, actions, T * 4, hipMemcpyHostToDevice, h->stream));
    EnvKernArgs ka = env_args(h, h->d_actions, -1, uniform_seats(opp_policy), auto_reset ? 1 : 0, h->d_reward, h->d_done, h->d_handf, h->d_terr,
                              obs ? (double *)h->d_export : nullptr);
    ka.A.obs_packed = d_packed;
    if (int rc = seat_launch(h, SEAT_KERNEL(k_env_step, env_grid(h), h->stream, ka))) return rc;
    // Busy from HERE on: if one of the copies below fails to queue, the earlier ones are already queued into the caller's buffers, and
    // pk_env_step_end is the caller's sanctioned way to wait for them (round 5 set the flag after the last copy: ADVICE r05).
    h->host_step = true;      // until pk_env_step_end: every entry point that reads or changes tables (another begin included) is PK_E_BUSY
    HIPCHK(h, hipMemcpyAsync(reward, h->d_reward, T * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(done, h->d_done, T, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(hand, h->d_handf, T, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(terr, h->d_terr, T, hipMemcpyDeviceToHost, h->stream));
    if (obs) HIPCHK(h, hipMemcpyAsync(obs, h->d_export, T * D * 8, hipMemcpyDeviceToHost, h->stream));
    if (obs_packed) HIPCHK(h, hipMemcpyAsync(obs_packed, d_packed, T * PB, hipMemcpyDeviceToHost, h->stream));
    return PK_OK;
}

int pk_env_step_end(pk_handle *h) {
    if (!h) return PK_E_INVALID_ARG;
    ON_DEVICE(h);
    if (!h->host_step) return h->fail(PK_E_INVALID_ARG, "pk_env_step_end: no pk_env_step_begin is waiting for it");
    h->host_step = false;     // (whatever the wait below returns, nothing is queued into the caller's buffers any more once it has)
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PK_OK;
}

#ifdef PK_PROFILE
// Diagnostic library only: read and clear the per-block cycle sums (slots: pk_device.hpp PF_*).
int pk_prof_read(pk_handle *h, unsigned long long *out) {
    if (!h || !out) return PK_E_INVALID_ARG;
    ON_DEVICE(h);
    if (!h->env_pending) FLUSH(h);   // (the counters themselves can be read while env steps are in flight)
    HIPCHK(h, hipMemcpyAsync(out, h->S.prof, PF_SLOTS * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemsetAsync(h->S.prof, 0, PF_SLOTS * 8, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PK_OK;
}
#endif

int pk_sync(pk_handle *h) {
    if (!h) return PK_E_INVALID_ARG;
    ON_DEVICE(h);
    if (!in_flight(h)) FLUSH(h);     // env steps in flight stay in flight: only wait for the launches made so far
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int b = 0; b < h->env_batches && h->env_batches > 1; ++b) HIPCHK(h, hipStreamSynchronize(h->env_streams[b]));
    return PK_OK;
}

// ---- snapshots (pokerl_hip.h "Snapshots"; kernels: pk_snapshot.hip)
static int snap_prepare(pk_handle *h) {   // the refusal word, the per-table marks and the event, on first use; the device is current
    if (!h->snap_word) HIPCHK(h, hipMalloc(&h->snap_word, 256));
    if (!h->snap_mark) HIPCHK(h, hipMalloc(&h->snap_mark, (size_t)h->T * 4));
    if (!h->snap_ev) HIPCHK(h, hipEventCreateWithFlags(&h->snap_ev, hipEventDisableTiming));
    return PK_OK;
}
static int snap_staging(pk_handle *h, size_t bytes, char **out) {   // grow-only, exactly as large as the largest call so far
    *out = (char *)h->snap_stage.reserve(bytes, bytes, h->stream);
    return *out ? PK_OK : h->fail(PK_E_OOM, "snapshot staging buffer", h->snap_stage.err);
}
static SnapHeader snap_header_of(const pk_handle *h, size_t m) {
    SnapHeader hd{};
    hd.magic = SNAP_MAGIC; hd.version = SNAP_VERSION; hd.num_players = (uint32_t)h->N; hd.m = m;
    for (int i = 0; i < PK_MAX_PLAYERS; ++i) hd.start_credits[i] = h->S.start_credits[i];
    hd.big_blind = h->S.big_blind; hd.small_blind = h->S.small_blind;
    return hd;
}
static bool snap_same_money(const pk_handle *a, const SnapHeader &b) {   // (start credits of unused seats are 0 on both sides)
    bool same = a->S.big_blind == b.big_blind && a->S.small_blind == b.small_blind;
    for (int i = 0; i < PK_MAX_PLAYERS; ++i) same = same && a->S.start_credits[i] == b.start_credits[i];
    return same;
}
// Reads the refusal word the check kernels queued on h->stream (waits for the stream); non-zero refusal bits fail the call.
static int snap_verdict(pk_handle *h, const char *call, uint32_t *word_out) {
    uint32_t w = 0;
    HIPCHK(h, hipMemcpyAsync(&w, h->snap_word, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (word_out) *word_out = w;
    if (!(w & ~SNAP_OVERLAP)) return PK_OK;
    std::string s = std::string(call) + ": refused, nothing written:";
    if (w & SNAP_BAD_SRC_INDEX) s += " a source table index is out of range;";
    if (w & SNAP_BAD_DST_INDEX) s += " a destination table index is out of range;";
    if (w & SNAP_DUP_DST) s += " a destination table is named twice;";
    if (w & SNAP_BAD_CURSOR) s += " a record's cursors are invalid (seat nibble >= N, turn > 4 or in-flight bits set);";
    if (w & SNAP_BAD_SEATS) s += " a record's seat masks use seats >= N or overlap;";
    if (w & SNAP_BAD_CARD) s += " a record holds a byte that is no card, or a card twice;";
    if (w & SNAP_BAD_MONEY) s += " a record holds money that is inf or NaN;";
    if (w & SNAP_BAD_VALID) s += " a record's valid-action mask has bit 7 set;";
    return h->fail(PK_E_INVALID_ARG, s.c_str());
}
// Checks an index array on the device: in range, and (dst) no table twice.
static int snap_check_tables(pk_handle *h, const int32_t *tables_d, size_t m, bool dst) {
    if (!tables_d) return PK_OK;
    if (dst) HIPCHK(h, hipMemsetAsync(h->snap_mark, 0, (size_t)h->T * 4, h->stream));
    HIPCHK(h, snap_check_idx(h->stream, tables_d, m, h->T, dst ? h->snap_mark : nullptr, 0, dst ? SNAP_BAD_DST_INDEX : SNAP_BAD_SRC_INDEX,
                             h->snap_word));
    return PK_OK;
}
static int snap_save(pk_handle *h, const int32_t *tables_d, size_t m, void *blob_d, const char *call) {
    if (!tables_d && m > (size_t)h->T) return h->fail(PK_E_INVALID_ARG, (std::string(call) + ": tables NULL and m > the handle's tables").c_str());
    if ((uintptr_t)blob_d & 7) return h->fail(PK_E_INVALID_ARG, (std::string(call) + ": blob must be 8-byte aligned").c_str());
    if (tables_d) {
        int rc = snap_prepare(h);
        if (rc) return rc;
        HIPCHK(h, hipMemsetAsync(h->snap_word, 0, 4, h->stream));
        if ((rc = snap_check_tables(h, tables_d, m, false))) return rc;
        if ((rc = snap_verdict(h, call, nullptr))) return rc;
    }
    SnapView blob;
    SnapPads pads;
    snap_layout(h->N, m, (char *)blob_d, &blob, &pads);
    HIPCHK(h, snap_copy(h->stream, SNAP_KIND_SAVE, snap_view_of_state(h->S), tables_d, blob, nullptr, h->N, m, Redeal{PK_OBSERVER_NONE, 0, 0, 0, 0},
                        snap_header_of(h, m), blob_d, pads));
    return PK_OK;
}
// May the blob that starts with `hd` be loaded into m tables of h?
static int snap_check_header(pk_handle *h, const SnapHeader &hd, size_t m, const char *call) {
    const std::string c(call);
    if (hd.magic != SNAP_MAGIC || hd.version != SNAP_VERSION) return h->fail(PK_E_INVALID_ARG, (c + ": not a snapshot of this format (magic / version)").c_str());
    if (hd.num_players != (uint32_t)h->N) return h->fail(PK_E_INVALID_ARG, (c + ": the blob holds tables of another number of seats").c_str());
    if (!snap_same_money(h, hd)) return h->fail(PK_E_INVALID_ARG, (c + ": the blob's start credits or blinds differ from the handle's").c_str());
    if (hd.m != m) return h->fail(PK_E_INVALID_ARG, (c + ": m differs from the blob's record count").c_str());
    if (m > (size_t)h->T) return h->fail(PK_E_INVALID_ARG, (c + ": more records than the handle has tables").c_str());
    return PK_OK;
}
// (the caller has checked the blob's header: snap_check_header)
static int snap_load(pk_handle *h, const int32_t *tables_d, size_t m, const void *blob_d, const char *call) {
    int rc = snap_prepare(h);
    if (rc) return rc;
    SnapView blob;
    snap_layout(h->N, m, (char *)const_cast<void *>(blob_d), &blob);
    HIPCHK(h, hipMemsetAsync(h->snap_word, 0, 4, h->stream));
    if ((rc = snap_check_tables(h, tables_d, m, true))) return rc;
    HIPCHK(h, snap_check_records(h->stream, blob, h->N, m, h->snap_word));
    if ((rc = snap_verdict(h, call, nullptr))) return rc;
    HIPCHK(h, snap_copy(h->stream, SNAP_KIND_LOAD, blob, nullptr, snap_view_of_state(h->S), tables_d, h->N, m, Redeal{PK_OBSERVER_NONE, 0, 0, 0, 0},
                        SnapHeader{}, nullptr, SnapPads{}));
    return PK_OK;
}

size_t pk_snapshot_bytes(int num_players, size_t m) {
    if (num_players < PK_MIN_PLAYERS || num_players > PK_MAX_PLAYERS) return 0;
    return snap_layout(num_players, m, nullptr, nullptr);
}

// The opening of the four save / load entry points (m == 0: nothing to do, once the handle has been flushed)
#define SNAP_ENTER(h, blob, m, call)                                                                      \
    if (!(h) || !(blob)) return (h) ? (h)->fail(PK_E_INVALID_ARG, call ": NULL blob") : PK_E_INVALID_ARG; \
    ON_DEVICE(h);                                                                                         \
    FLUSH(h);                                                                                             \
    if ((m) == 0) return PK_OK

int pk_save_tables_d(pk_handle *h, const int32_t *tables_d, size_t m, void *blob_d) {
    SNAP_ENTER(h, blob_d, m, "pk_save_tables_d");
    return snap_save(h, tables_d, m, blob_d, "pk_save_tables_d");
}

int pk_load_tables_d(pk_handle *h, const int32_t *tables_d, size_t m, const void *blob_d) {
    SNAP_ENTER(h, blob_d, m, "pk_load_tables_d");
    if ((uintptr_t)blob_d & 7) return h->fail(PK_E_INVALID_ARG, "pk_load_tables_d: blob must be 8-byte aligned");
    SnapHeader hd{};
    HIPCHK(h, hipMemcpyAsync(&hd, blob_d, sizeof(hd), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (int rc = snap_check_header(h, hd, m, "pk_load_tables_d")) return rc;
    return snap_load(h, tables_d, m, blob_d, "pk_load_tables_d");
}

int pk_save_tables(pk_handle *h, const int32_t *tables, size_t m, void *blob) {
    SNAP_ENTER(h, blob, m, "pk_save_tables");
    if (!tables && m > (size_t)h->T) return h->fail(PK_E_INVALID_ARG, "pk_save_tables: tables NULL and m > the handle's tables");   // (before staging)
    Stage g;
    const int idx = g.in(tables, m * 4), rec = g.out(blob, pk_snapshot_bytes(h->N, m));
    int rc = snap_staging(h, g.total, &g.base);
    if (rc) return rc;
    HIPCHK(h, g.upload(h->stream));
    if ((rc = snap_save(h, g.at<int32_t>(idx), m, g.at<char>(rec), "pk_save_tables"))) return rc;
    HIPCHK(h, g.download(h->stream));
    return PK_OK;
}

int pk_load_tables(pk_handle *h, const int32_t *tables, size_t m, const void *blob) {
    SNAP_ENTER(h, blob, m, "pk_load_tables");
    // the header first, from host memory: it says how many bytes the caller's blob holds
    SnapHeader hd;
    memcpy(&hd, blob, sizeof(hd));
    int rc = snap_check_header(h, hd, m, "pk_load_tables");
    if (rc) return rc;
    Stage g;
    const int idx = g.in(tables, m * 4), rec = g.in(blob, pk_snapshot_bytes(h->N, m));
    if ((rc = snap_staging(h, g.total, &g.base))) return rc;
    HIPCHK(h, g.upload(h->stream));
    if ((rc = snap_load(h, g.at<int32_t>(idx), m, g.at<char>(rec), "pk_load_tables"))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PK_OK;
}

int pk_clone_tables_d(pk_handle *dst, const int32_t *dst_tables_d, pk_handle *src, const int32_t *src_tables_d, size_t m, int observer,
                      uint64_t nonce) {
    if (!dst || !src) {
        if (dst) return dst->fail(PK_E_INVALID_ARG, "pk_clone_tables_d: NULL source handle");
        g_err = "pk_clone_tables_d: NULL destination handle";
        return PK_E_INVALID_ARG;
    }
    if (dst->device != src->device) return dst->fail(PK_E_INVALID_ARG, "pk_clone_tables_d: the handles are on different devices (save / load through a blob instead)");
    if (dst->N != src->N) return dst->fail(PK_E_INVALID_ARG, "pk_clone_tables_d: the handles have different numbers of seats");
    if (!snap_same_money(dst, snap_header_of(src, 0))) return dst->fail(PK_E_INVALID_ARG, "pk_clone_tables_d: the handles' start credits or blinds differ");
    if (observer < PK_OBSERVER_ACTIVE || observer >= dst->N) return dst->fail(PK_E_INVALID_ARG, "pk_clone_tables_d: observer must be -2, -1 or a seat");
    ON_DEVICE(dst);
    if (src != dst) {
        const int rc = flush(src);
        if (rc) return dst->fail(rc, src->err.c_str());
    }
    FLUSH(dst);
    if (m == 0) return PK_OK;
    if (m > (size_t)dst->T) return dst->fail(PK_E_INVALID_ARG, "pk_clone_tables_d: more destinations than the handle has tables");
    if (!src_tables_d && m > (size_t)src->T) return dst->fail(PK_E_INVALID_ARG, "pk_clone_tables_d: src_tables_d NULL and m > the source's tables");
    int rc = snap_prepare(dst);
    if (rc) return rc;
    if (src != dst) {   // the clone reads what src's stream has queued so far
        HIPCHK(dst, hipEventRecord(dst->snap_ev, src->stream));
        HIPCHK(dst, hipStreamWaitEvent(dst->stream, dst->snap_ev, 0));
    }
    // Destinations: in range, none twice (marks).  Sources: in range; within one handle also whether one of them is a destination -- then
    // the reads are staged through a blob first, so that the result is that of all reads before any write.
    const bool marks = dst_tables_d || src == dst;   // (tables 0 .. m-1 of another handle need neither check)
    HIPCHK(dst, hipMemsetAsync(dst->snap_word, 0, 4, dst->stream));
    if (marks) {
        HIPCHK(dst, hipMemsetAsync(dst->snap_mark, 0, (size_t)dst->T * 4, dst->stream));
        HIPCHK(dst, snap_check_idx(dst->stream, dst_tables_d, m, dst->T, dst->snap_mark, 0, SNAP_BAD_DST_INDEX, dst->snap_word));
    }
    HIPCHK(dst, snap_check_idx(dst->stream, src_tables_d, m, src->T, src == dst ? dst->snap_mark : nullptr, 1, SNAP_BAD_SRC_INDEX, dst->snap_word));
    uint32_t word = 0;
    if ((rc = snap_verdict(dst, "pk_clone_tables_d", &word))) return rc;
    const Redeal rd{observer, dst->S.key0, dst->S.key1, dst->S.table_id_base, nonce};
    if (word & SNAP_OVERLAP) {
        char *stage = nullptr;
        if ((rc = snap_staging(dst, pk_snapshot_bytes(dst->N, m), &stage))) return rc;
        SnapView blob;
        SnapPads pads;
        snap_layout(dst->N, m, stage, &blob, &pads);
        HIPCHK(dst, snap_copy(dst->stream, SNAP_KIND_SAVE, snap_view_of_state(src->S), src_tables_d, blob, nullptr, dst->N, m, rd, snap_header_of(src, m), stage,
                              pads));
        HIPCHK(dst, snap_copy(dst->stream, SNAP_KIND_CLONE, blob, nullptr, snap_view_of_state(dst->S), dst_tables_d, dst->N, m, rd, SnapHeader{}, nullptr,
                              SnapPads{}));
    } else {
        HIPCHK(dst, snap_copy(dst->stream, SNAP_KIND_CLONE, snap_view_of_state(src->S), src_tables_d, snap_view_of_state(dst->S), dst_tables_d, dst->N, m, rd,
                              SnapHeader{}, nullptr, SnapPads{}));
    }
    if (src != dst) {   // src's later work waits for the clone's reads
        HIPCHK(dst, hipEventRecord(dst->snap_ev, dst->stream));
        HIPCHK(dst, hipStreamWaitEvent(src->stream, dst->snap_ev, 0));
    }
    return PK_OK;
}

// ---- standalone judger ops (no handle)
// Grow-only device scratch of the host-buffer judger calls, one per device: no hipMalloc / hipFree per call.
static std::mutex g_scratch_mu;
static DevBuf g_scratch[PK_MAX_DEVICES];
// Caller holds g_scratch_mu, has the device current and waits for its own work on `stream` before it lets go of the lock.
static char *scratch(int device, size_t bytes, hipStream_t stream) { return (char *)g_scratch[device].reserve(bytes, with_headroom(bytes, 2), stream, true); }

// pk_eval_hands(_d)'s launch: the table path (k_eval_hands_tab); the register evaluator if the table could not be allocated.
// tab: eval7_table(device), fetched by the caller BEFORE it takes g_scratch_mu.
static void launch_eval_hands(const uint32_t *tab, const uint8_t *cards_d, const uint8_t *ncards_d, size_t m, uint8_t *rank_d, uint32_t *kick_d,
                              uint8_t *nkick_d, hipStream_t stream) {
    if (tab) {
        const size_t chunks = (m + EVAL_TAB_BLOCK - 1) / EVAL_TAB_BLOCK;      // every workgroup copies the 32 KB table: no more of them than have hands
        const unsigned grid = (unsigned)(chunks < 256 * 8 ? chunks : 256 * 8);   // four resident per CU (LDS), two rounds; grid-stride over the rest
        if (ncards_d) hipLaunchKernelGGL(k_eval_hands_tab<true>, dim3(grid), dim3(EVAL_TAB_BLOCK), 0, stream, cards_d, ncards_d, m, rank_d, kick_d, nkick_d, tab);
        else hipLaunchKernelGGL(k_eval_hands_tab<false>, dim3(grid), dim3(EVAL_TAB_BLOCK), 0, stream, cards_d, ncards_d, m, rank_d, kick_d, nkick_d, tab);
    } else {
        hipLaunchKernelGGL(k_eval_hands, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, cards_d, ncards_d, m, rank_d, kick_d, nkick_d);
    }
}

int pk_eval_hands_d(int device, const uint8_t *cards_d, const uint8_t *ncards_d, size_t m, uint8_t *rank_d, uint32_t *kick_d,
                    uint8_t *nkick_d, void *stream) {
    if (!cards_d || !rank_d || !kick_d) return g_fail(PK_E_INVALID_ARG, "pk_eval_hands_d: NULL buffer");
    ON_DEVICE_INDEX("pk_eval_hands_d", device, INT_MAX);
    if (m == 0) return PK_OK;
    launch_eval_hands(eval7_table(device, (hipStream_t)stream), cards_d, ncards_d, m, rank_d, kick_d, nkick_d, (hipStream_t)stream);   // (a first call builds the table on the CALLER's stream)
    if (hipGetLastError() != hipSuccess) return g_fail(PK_E_HIP, "pk_eval_hands_d: launch failed");
    return PK_OK;
}

int pk_eval_hands(int device, const uint8_t *cards, const uint8_t *ncards, size_t m, uint8_t *rank, uint32_t *kick,
                  uint8_t *nkick) {
    if (!cards || !rank || !kick) return g_fail(PK_E_INVALID_ARG, "pk_eval_hands: NULL buffer");
    ON_DEVICE_INDEX("pk_eval_hands", device, PK_MAX_DEVICES);
    if (m == 0) return PK_OK;
    const uint32_t *tab = eval7_table(device);   // (takes g_scratch_mu itself)
    std::lock_guard<std::mutex> lock(g_scratch_mu);
    Stage g;
    const int c = g.in(cards, m * 7), nc = g.in(ncards, m), r = g.out(rank, m), k = g.out(kick, m * 4), nk = g.out(nkick, m);
    if (!(g.base = scratch(device, g.total, 0))) return g_fail(PK_E_OOM, "pk_eval_hands: out of device memory");
    const hipError_t e = g.run(0, [&] { launch_eval_hands(tab, g.at<uint8_t>(c), g.at<uint8_t>(nc), m, g.at<uint8_t>(r), g.at<uint32_t>(k), g.at<uint8_t>(nk), 0); return hipGetLastError(); });
    return e == hipSuccess ? PK_OK : g_fail(PK_E_HIP, "pk_eval_hands", e);
}

int pk_compare_rankings(int device, const uint8_t *rank, const uint32_t *kick, int n, size_t m, uint8_t *onehot) {
    if (!rank || !kick || !onehot || n < 1 || n > 32) return g_fail(PK_E_INVALID_ARG, "pk_compare_rankings: bad argument (1 <= n <= 32)");
    ON_DEVICE_INDEX("pk_compare_rankings", device, PK_MAX_DEVICES);
    if (m == 0) return PK_OK;
    std::lock_guard<std::mutex> lock(g_scratch_mu);
    const size_t cnt = m * (size_t)n;
    Stage g;
    const int k = g.in(kick, cnt * 4), r = g.in(rank, cnt), o = g.out(onehot, cnt);
    if (!(g.base = scratch(device, g.total, 0))) return g_fail(PK_E_OOM, "pk_compare_rankings: out of device memory");
    const hipError_t e = g.run(0, [&] {
        hipLaunchKernelGGL(k_compare, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, g.at<uint8_t>(r), (const uint32_t *)g.at<uint32_t>(k), n, m, g.at<uint8_t>(o));
        return hipGetLastError();
    });
    return e == hipSuccess ? PK_OK : g_fail(PK_E_HIP, "pk_compare_rankings", e);
}

// The 32 KB table of the table-driven evaluator (eval7_tab), one per device, built on first use.
static DevBuf g_eval_tab[PK_MAX_DEVICES];
static const uint32_t *eval7_table(int device, hipStream_t stream) {   // the device is current
    if (device < 0 || device >= PK_MAX_DEVICES) return nullptr;
    std::lock_guard<std::mutex> lock(g_scratch_mu);
    DevBuf &t = g_eval_tab[device];
    if (!t.alive()) {   // (not yet there, or the device was reset: build it)
        t = DevBuf{};
        uint32_t *p = (uint32_t *)t.reserve(EVAL7_TAB_WORDS * 4, EVAL7_TAB_WORDS * 4, stream, true);
        if (!p) return nullptr;
        hipLaunchKernelGGL(k_make_eval7_tab, dim3(EVAL7_TAB_WORDS / 256), dim3(256), 0, stream, p);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) { t.drop(); return nullptr; }
    }
    return (const uint32_t *)t.p;
}

static int launch_eval7(int device, const uint64_t *hands_d, size_t m, uint32_t *out_d, int distinct) {
    const unsigned grid = 256 * 16;  // 16 workgroups per CU, grid-stride over the rest
    const bool vec = (((uintptr_t)hands_d & 15) | ((uintptr_t)out_d & 7)) == 0;  // 16-byte loads / 8-byte stores need it
    const uint32_t *tab = distinct ? eval7_table(device) : nullptr;
    if (tab) {   // four 512-thread workgroups per CU (LDS: 4 x 32 KB), two rounds of them
        const size_t want = (m / 2 + 511) / 512;     // every workgroup copies the 32 KB table: no more of them than have hands
        const unsigned gridx = (unsigned)(want < 1 ? 1 : (want < 256 * 32 ? want : 256 * 32));
        if (vec) hipLaunchKernelGGL(k_eval7_tab_stream<true>, dim3(gridx), dim3(512), 0, 0, hands_d, m, out_d, tab);
        else hipLaunchKernelGGL(k_eval7_tab_stream<false>, dim3(gridx), dim3(512), 0, 0, hands_d, m, out_d, tab);
    } else if (distinct) {
        if (vec) hipLaunchKernelGGL((k_eval7_stream<true, true>), dim3(grid), dim3(256), 0, 0, hands_d, m, out_d);
        else hipLaunchKernelGGL((k_eval7_stream<true, false>), dim3(grid), dim3(256), 0, 0, hands_d, m, out_d);
    } else {
        if (vec) hipLaunchKernelGGL((k_eval7_stream<false, true>), dim3(grid), dim3(256), 0, 0, hands_d, m, out_d);
        else hipLaunchKernelGGL((k_eval7_stream<false, false>), dim3(grid), dim3(256), 0, 0, hands_d, m, out_d);
    }
    return hipGetLastError() == hipSuccess ? PK_OK : PK_E_HIP;
}

int pk_eval7_d(int device, const uint64_t *hands_d, size_t m, uint32_t *out_d, int distinct) {
    if (!hands_d || !out_d || ((uintptr_t)hands_d & 7) || ((uintptr_t)out_d & 3)) return g_fail(PK_E_INVALID_ARG, "pk_eval7_d: NULL or misaligned buffer");
    ON_DEVICE_INDEX("pk_eval7_d", device, INT_MAX);
    if (m == 0) return PK_OK;
    if (launch_eval7(device, hands_d, m, out_d, distinct) != PK_OK || hipDeviceSynchronize() != hipSuccess) return g_fail(PK_E_HIP, "pk_eval7_d: launch failed");
    return PK_OK;
}

int pk_make_hands_d(int device, uint64_t seed, size_t m, uint64_t *hands_d) {
    if (!hands_d) return g_fail(PK_E_INVALID_ARG, "pk_make_hands_d: NULL buffer");
    ON_DEVICE_INDEX("pk_make_hands_d", device, INT_MAX);
    if (m == 0) return PK_OK;
    Hot H{};
    H.key0 = (uint32_t)seed; H.key1 = (uint32_t)(seed >> 32);
    hipLaunchKernelGGL(k_make_hands, dim3(256 * 16), dim3(256), 0, 0, H, m, hands_d);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return g_fail(PK_E_HIP, "pk_make_hands_d: launch failed");
    return PK_OK;
}

int pk_time_eval7_d(int device, const uint64_t *hands_d, size_t m, uint32_t *out_d, int distinct, int reps, double *ms_per_pass) {
    if (!hands_d || !out_d || !ms_per_pass || reps < 1) return g_fail(PK_E_INVALID_ARG, "pk_time_eval7_d: bad argument");
    ON_DEVICE_INDEX("pk_time_eval7_d", device, INT_MAX);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
        if (e0) (void)hipEventDestroy(e0);
        return g_fail(PK_E_HIP, "hipEventCreate failed");
    }
    launch_eval7(device, hands_d, m, out_d, distinct);  // warm (instruction cache, clocks)
    (void)hipEventRecord(e0, 0);
    for (int r = 0; r < reps; ++r) launch_eval7(device, hands_d, m, out_d, distinct);
    (void)hipEventRecord(e1, 0);
    hipError_t e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (e != hipSuccess) return g_fail(PK_E_HIP, "pk_time_eval7_d", e);
    *ms_per_pass = (double)ms / reps;
    return PK_OK;
}

// Test hook (declared in pokerl_hip.h as part of the judger surface): values rank<<20|kick of all 7-card hands whose
// two lowest canonical indices are (a, b), lexicographic order.  out holds C(51-b, 5) words.
int pk_eval7_prefix(int device, int a, int b, int fast, uint32_t *out, size_t *count_out) {
    if (!out || a < 0 || b <= a || b > 51) return g_fail(PK_E_INVALID_ARG, "pk_eval7_prefix: bad argument");
    ON_DEVICE_INDEX("pk_eval7_prefix", device, PK_MAX_DEVICES);
    int n = 51 - b;
    size_t count = n >= 5 ? (size_t)n * (n - 1) * (n - 2) * (n - 3) * (n - 4) / 120 : 0;
    if (count_out) *count_out = count;
    if (!count) return PK_OK;
    const uint32_t *tab = (fast == 2 || fast == 4) ? eval7_table(device) : nullptr;   // (takes g_scratch_mu itself)
    if ((fast == 2 || fast == 4) && !tab) return g_fail(PK_E_OOM, "pk_eval7_prefix: out of device memory");
    std::lock_guard<std::mutex> lock(g_scratch_mu);
    uint32_t *d = (uint32_t *)scratch(device, count * 4, 0);
    if (!d) return g_fail(PK_E_OOM, "pk_eval7_prefix: out of device memory");
    hipLaunchKernelGGL(k_eval7_prefix, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, 0, a, b, fast, (uint32_t)count, d, tab);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out, d, count * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return g_fail(PK_E_HIP, "pk_eval7_prefix", e);
    return PK_OK;
}

// ---- the equity family's work space of the device forms, which run asynchronously on the CALLER's stream: one grow-only hipMalloc'ed buffer
// per (device, stream), reused by the next call on that stream -- stream order makes that safe -- and at most EQ_WS_STREAMS of them per device
// (the least recently used one is freed for a new stream; hipFree waits for the device, so work still queued on it is not cut short).  NOT the
// stream-ordered allocator: with hipMallocAsync / hipFreeAsync every call that followed a synchronisation got a fresh mapping, and on
// such a mapping the enumeration kernel found the task count still zero -- every third call of a 4 096-spot loop returned all-zero
// counts (measured, ROCm 7.2).
static const int EQ_WS_STREAMS = 8;
struct EqStreamWs { hipStream_t stream; DevBuf buf; uint64_t used; };
static std::mutex g_eq_ws_mu;
static std::vector<EqStreamWs> g_eq_ws[PK_MAX_DEVICES];
static uint64_t g_eq_ws_clock;
static void *eq_stream_ws(int device, hipStream_t st, size_t bytes) {   // the device is current and < PK_MAX_DEVICES
    std::lock_guard<std::mutex> lock(g_eq_ws_mu);
    auto &v = g_eq_ws[device];
    for (size_t i = 0; i < v.size();)            // (other streams' buffers that vanished with a device reset are forgotten, not freed; reserve sees to this stream's)
        if (v[i].stream != st && !v[i].buf.alive()) v.erase(v.begin() + i); else ++i;
    EqStreamWs *hit = nullptr;
    for (auto &x : v) if (x.stream == st) hit = &x;
    if (!hit) {
        if ((int)v.size() >= EQ_WS_STREAMS) {
            size_t lru = 0;
            for (size_t i = 1; i < v.size(); ++i) if (v[i].used < v[lru].used) lru = i;
            v[lru].buf.drop();
            v.erase(v.begin() + lru);
        }
        v.push_back(EqStreamWs{st, DevBuf{}, 0});
        hit = &v.back();
    }
    hit->used = ++g_eq_ws_clock;
    return hit->buf.reserve(bytes, with_headroom(bytes, 4), st, true);   // (too small: the calls queued on it so far finish before it goes)
}

// ---- showdown equity (pokerl_hip.h "Showdown equity"; kernels: pk_equity.hip) and, after it, the rest of the equity family.  Every family
// comes in the same four forms, and each form is written ONCE here: an entry point checks its arguments, names its
// staging pieces and its work-space size, and hands a lambda that queues its kernels to the form's skeleton.
// The per-device table a family's kernels read, handed to its launch as `tab`: none, the evaluator table, or the pre-flop matchup
// table (pfm_table, further down: win [1326][1326], then tie).  A first call builds it on the CALLER's stream.
enum { EQ_TAB_NONE = 0, EQ_TAB_EVAL = 1, EQ_TAB_PREFLOP = 2 };
static const uint32_t *pfm_table(int device, hipStream_t stream);
static const uint32_t *eq_resident(int need, int device, hipStream_t st) {
    return need == EQ_TAB_PREFLOP ? pfm_table(device, st) : (need ? eval7_table(device, st) : nullptr);
}
static const char *eq_resident_text(int need) { return need == EQ_TAB_PREFLOP ? ": out of device memory (pre-flop matchup table)" : ": out of device memory (evaluator table)"; }

extern "C++" {   // (templates)
static int eq_fail(int code, const char *call, const char *what, hipError_t e = hipSuccess) { return g_fail(code, (std::string(call) + what).c_str(), e); }

// The device form: asynchronous on the CALLER's stream, every array in device memory; the work space is that stream's (above).
// launch(st, tab, work) queues the kernels; tab is the table need_table names (EQ_TAB_*), NULL for EQ_TAB_NONE.
template <typename F>
static int eq_call_d(const char *call, int device, void *stream, size_t m, int need_table, size_t work_bytes, F launch) {
    ON_DEVICE_INDEX(call, device, PK_MAX_DEVICES);   // (the evaluator table is kept per device index below PK_MAX_DEVICES)
    if (m == 0) return PK_OK;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t *tab = eq_resident(need_table, device, st);   // (a first call builds the table on the CALLER's stream)
    if (need_table && !tab) return eq_fail(PK_E_OOM, call, eq_resident_text(need_table));
    char *work = (char *)eq_stream_ws(device, st, work_bytes);
    if (!work) return eq_fail(PK_E_OOM, call, ": out of device memory (work space)");
    const hipError_t e = launch(st, tab, work);
    if (e != hipSuccess) return eq_fail(PK_E_HIP, call, ": launch failed", e);
    return PK_OK;
}

// The host form: the caller's host arrays, staged in ONE buffer (g's pieces: inputs, outputs, then the work space) of the judger arena on a
// pooled stream; returns when the outputs are in the caller's arrays.  launch(st, tab, work) as above, on g.at<T>(piece).
template <typename F>
static int eq_call_host(const char *call, int device, size_t m, int need_table, Stage &g, size_t work_bytes, F launch) {
    ON_DEVICE_INDEX(call, device, PK_MAX_DEVICES);
    if (m == 0) return PK_OK;
    hipStream_t st = nullptr;
    if (stream_acquire(device, &st) != hipSuccess) { (void)hipGetLastError(); return eq_fail(PK_E_HIP, call, ": no stream"); }
    const uint32_t *tab = eq_resident(need_table, device, st);   // (takes g_scratch_mu itself)
    int rc = PK_OK;
    if (need_table && !tab) rc = eq_fail(PK_E_OOM, call, eq_resident_text(need_table));
    else {
        std::lock_guard<std::mutex> lock(g_scratch_mu);
        const int work = g.add(work_bytes);
        if (!(g.base = scratch(device, g.total, st))) rc = eq_fail(PK_E_OOM, call, ": out of device memory");
        else {
            const hipError_t e = g.run(st, [&] { return launch(st, tab, g.at<char>(work)); });
            if (e != hipSuccess) { (void)hipStreamSynchronize(st); rc = g_fail(PK_E_HIP, call, e); }   // (the lock is held until what was queued is done)
        }
    }
    stream_release(device, st);
    return rc;
}

// The two table forms read the handle's own state on the handle's stream; their work space is the handle's grow-only staging buffer.  What
// they share once that is there: the table need_table names (EQ_TAB_*), the handle's state as EqTables, launch(tab, tables, work).
template <typename F>
static int eq_table_launch(pk_handle *h, const char *call, const int32_t *tables_d, int need_table, char *work, F launch) {
    const uint32_t *tab = eq_resident(need_table, h->device, h->stream);
    if (!tab && need_table == EQ_TAB_PREFLOP) return h->fail(PK_E_OOM, (std::string(call) + eq_resident_text(need_table)).c_str());
    if (!tab && need_table) {
        std::string family(call);                    // (this text has always named the family, without the device form's _d)
        if (family.size() > 2 && family.compare(family.size() - 2, 2, "_d") == 0) family.resize(family.size() - 2);
        return h->fail(PK_E_OOM, (family + ": out of device memory (evaluator table)").c_str());
    }
    const EqTables t{h->S.cards, h->S.seat_states, h->S.cursors, tables_d, h->T};
    const hipError_t e = launch(tab, t, work);
    if (e != hipSuccess) return h->fail(PK_E_HIP, (std::string(call) + ": launch failed").c_str(), e);
    return PK_OK;
}
// The device form: tables_d and the outputs in device memory, asynchronous on the handle's stream (m == 0: nothing to do, once the handle has
// been flushed)
template <typename F>
static int eq_table_call_d(pk_handle *h, const char *call, const int32_t *tables_d, size_t m, int need_table, size_t work_bytes, F launch) {
    ON_DEVICE(h);
    FLUSH_READER(h);
    if (m == 0) return PK_OK;
    char *work = nullptr;
    if (int rc = snap_staging(h, work_bytes, &work)) return rc;
    return eq_table_launch(h, call, tables_d, need_table, work, launch);
}
// The host form: g's pieces (inputs, outputs), then the table indices and the work space, staged as the host form above stages them
template <typename F>
static int eq_table_call(pk_handle *h, const char *call, const int32_t *tables, size_t m, int need_table, Stage &g, size_t work_bytes, F launch) {
    ON_DEVICE(h);
    FLUSH_READER(h);
    if (m == 0) return PK_OK;
    const int idx = g.in(tables, m * 4), work = g.add(work_bytes);
    if (int rc = snap_staging(h, g.total, &g.base)) return rc;
    HIPCHK(h, g.upload(h->stream));
    if (int rc = eq_table_launch(h, call, g.at<int32_t>(idx), need_table, g.at<char>(work), launch)) return rc;
    HIPCHK(h, g.download(h->stream));
    return PK_OK;
}
}  // extern "C++"

// The argument checks, made before the device is looked at.  Each gives the text its refusal ends in, or NULL; a family's check asks them in
// the order its entry points always have.  EQ_REFUSE returns PK_E_INVALID_ARG with "<call><text>" (fail: g_fail, or the handle's).
#define EQ_REFUSE(fail, call, check) \
    if (const char *why_ = (check)) return fail(PK_E_INVALID_ARG, (std::string(call) + why_).c_str())
static const size_t EQ_MAX_SPOTS = (size_t)1 << 31;
static const char *eq_bad_m(size_t m) { return m >= EQ_MAX_SPOTS ? ": m >= 2^31" : nullptr; }
static const char *eq_bad_spots(int num_players, size_t m) {
    return num_players < PK_MIN_PLAYERS || num_players > PK_MAX_PLAYERS || m >= EQ_MAX_SPOTS ? ": num_players outside 2 .. 16, or m >= 2^31" : nullptr;
}
static const char *eq_null(size_t m, bool given, const char *text = ": NULL input buffer") { return m && !given ? text : nullptr; }
// The device counts a call's tasks in 32 bits: a call whose worst case (every spot pre-flop) does not fit is refused, not wrapped.
static const char *eq_bad_tasks(size_t worst_case) {
    return worst_case > EQ_TASKS_MAX ? ": too many spots for one call (the worst-case task count must fit 32 bits: split the batch)" : nullptr;
}
static const char *eqs_bad_samples(uint32_t samples) { return samples == 0 || samples > EQS_SAMPLES_MAX ? ": samples outside 1 .. 2^24" : nullptr; }
static const char *eqs_bad_tasks(size_t m, uint32_t samples) {
    return eqs_task_bound(m, samples) > EQ_TASKS_MAX ? ": m * ceil(samples / 64) must fit 32 bits: split the batch" : nullptr;
}
static const char *eqw_bad_ranges(const uint16_t *weights, uint32_t num_ranges) {
    if (num_ranges > (uint32_t)EQW_MAX_RANGES) return ": num_ranges above PK_EQW_MAX_RANGES (16)";
    return num_ranges && !weights ? ": NULL weights with num_ranges > 0" : nullptr;
}
static const char *hist_bad_bins(int nbins) { return nbins < 1 || nbins > PK_EQ_HIST_MAX_BINS ? ": nbins must be 1 .. PK_EQ_HIST_MAX_BINS (32)" : nullptr; }
// whose eyes a table form looks through: a seat, the active player, or -- for sampled equity alone -- nobody's
static bool eq_observes(int observer, int N) { return observer == PK_OBSERVER_ACTIVE || (observer >= 0 && observer < N); }
static const char *eqs_bad_observer(int observer, int N) {
    return observer != PK_OBSERVER_NONE && !eq_observes(observer, N) ? ": observer outside {-2, -1, 0 .. N-1}" : nullptr;
}
static const char *eqw_bad_observer(int observer, int N) {
    return !eq_observes(observer, N) ? ": observer outside {-2, 0 .. N-1} (PK_OBSERVER_NONE: nothing would be hidden)" : nullptr;
}
static const char *eqr_bad_observer(int observer, int N) {
    return !eq_observes(observer, N) ? ": observer outside {-2, 0 .. N-1} (a hidden hand needs somebody to be hidden from)" : nullptr;
}

static const char *eq_check(int num_players, size_t m, bool inputs) {
    if (const char *why = eq_bad_spots(num_players, m)) return why;
    if (const char *why = eq_null(m, inputs)) return why;
    return eq_bad_tasks(eq_task_cap(m, eq_lpt(m), 50));
}
static const char *eq_table_check(const pk_handle *h, size_t m) {
    if (const char *why = eq_bad_m(m)) return why;
    return eq_bad_tasks(eq_task_cap(m, eq_lpt(m), 52 - 2 * h->N));
}

int pk_equity_d(int device, int num_players, size_t m, const uint8_t *holes_d, const uint8_t *board_d, const uint8_t *nboard_d,
                const uint16_t *live_d, uint32_t *win_d, uint32_t *tie_d, uint64_t *share_d, uint32_t *boards_d, uint8_t *status_d, void *stream) {
    const char *call = "pk_equity_d";
    EQ_REFUSE(g_fail, call, eq_check(num_players, m, holes_d && board_d && nboard_d && live_d));
    const int N = num_players, lpt = eq_lpt(m);
    return eq_call_d(call, device, stream, m, EQ_TAB_EVAL, eq_layout(N, m, lpt, 50, nullptr, nullptr), [&](hipStream_t st, const uint32_t *tab, char *work) {
        EqWork w;
        eq_layout(N, m, lpt, 50, work, &w);
        const EqSpots spots{holes_d, board_d, nboard_d, live_d};
        return eq_launch(st, tab, &spots, nullptr, N, m, EqOut{win_d, tie_d, share_d, boards_d, status_d}, w, lpt);
    });
}

int pk_equity(int device, int num_players, size_t m, const uint8_t *holes, const uint8_t *board, const uint8_t *nboard, const uint16_t *live,
              uint32_t *win, uint32_t *tie, uint64_t *share, uint32_t *boards, uint8_t *status) {
    const char *call = "pk_equity";
    EQ_REFUSE(g_fail, call, eq_check(num_players, m, holes && board && nboard && live));
    const int N = num_players, lpt = eq_lpt(m);
    Stage g;
    const int ho = g.in(holes, m * N * 2), bo = g.in(board, m * 5), nb = g.in(nboard, m), lv = g.in(live, m * 2);
    const EqStagedOut out(g, N, m, win, tie, share, boards, status);
    return eq_call_host(call, device, m, EQ_TAB_EVAL, g, eq_layout(N, m, lpt, 50, nullptr, nullptr), [&](hipStream_t st, const uint32_t *tab, char *work) {
        EqWork w;
        eq_layout(N, m, lpt, 50, work, &w);
        const EqSpots spots{g.at<uint8_t>(ho), g.at<uint8_t>(bo), g.at<uint8_t>(nb), g.at<uint16_t>(lv)};
        return eq_launch(st, tab, &spots, nullptr, N, m, out.at(g), w, lpt);
    });
}

int pk_table_equity_d(pk_handle *h, const int32_t *tables_d, size_t m, uint32_t *win_d, uint32_t *tie_d, uint64_t *share_d, uint32_t *boards_d,
                      uint8_t *status_d) {
    if (!h) return PK_E_INVALID_ARG;
    const char *call = "pk_table_equity_d";
    EQ_REFUSE(h->fail, call, eq_table_check(h, m));
    const int N = h->N, lpt = eq_lpt(m), pool = 52 - 2 * N;
    return eq_table_call_d(h, call, tables_d, m, EQ_TAB_EVAL, eq_layout(N, m, lpt, pool, nullptr, nullptr), [&](const uint32_t *tab, const EqTables &t, char *work) {
        EqWork w;
        eq_layout(N, m, lpt, pool, work, &w);
        return eq_launch(h->stream, tab, nullptr, &t, N, m, EqOut{win_d, tie_d, share_d, boards_d, status_d}, w, lpt);
    });
}

int pk_table_equity(pk_handle *h, const int32_t *tables, size_t m, uint32_t *win, uint32_t *tie, uint64_t *share, uint32_t *boards,
                    uint8_t *status) {
    if (!h) return PK_E_INVALID_ARG;
    const char *call = "pk_table_equity";
    EQ_REFUSE(h->fail, call, eq_table_check(h, m));
    const int N = h->N, lpt = eq_lpt(m), pool = 52 - 2 * N;
    Stage g;
    const EqStagedOut out(g, N, m, win, tie, share, boards, status);
    return eq_table_call(h, call, tables, m, EQ_TAB_EVAL, g, eq_layout(N, m, lpt, pool, nullptr, nullptr), [&](const uint32_t *tab, const EqTables &t, char *work) {
        EqWork w;
        eq_layout(N, m, lpt, pool, work, &w);
        return eq_launch(h->stream, tab, nullptr, &t, N, m, out.at(g), w, lpt);
    });
}

// ---- showdown EV in chips (pokerl_hip.h "Showdown EV"; kernels: pk_equity_ev.hip).  The work space also holds the level table, the bets, the
// amounts and -- when the caller does not ask for `share` -- the share counters.
struct EvStagedOut {
    int share, level_seat, amount, ev, boards, status;
    EvStagedOut(Stage &g, int N, size_t m, uint64_t *share, uint8_t *level_seat, double *amount, double *ev, uint32_t *boards, uint8_t *status)
        : share(g.out(share, m * N * N * 8)), level_seat(g.out(level_seat, m * N)), amount(g.out(amount, m * N * 8)), ev(g.out(ev, m * N * 8)),
          boards(g.out(boards, m * 4)), status(g.out(status, m)) {}
    EvOut at(const Stage &g) const {
        return EvOut{g.at<uint64_t>(share), g.at<uint8_t>(level_seat), g.at<double>(amount), g.at<double>(ev), g.at<uint32_t>(boards), g.at<uint8_t>(status)};
    }
};
static const char *ev_check(int num_players, size_t m, bool inputs_and_status) {
    if (const char *why = eq_bad_spots(num_players, m)) return why;
    if (const char *why = eq_null(m, inputs_and_status, ": NULL input buffer or NULL status")) return why;
    return eq_bad_tasks(ev_task_cap(num_players, m, eq_lpt(m), 50));
}
static const char *ev_table_check(const pk_handle *h, size_t m, const uint8_t *status) {
    if (const char *why = eq_bad_m(m)) return why;
    if (const char *why = eq_null(m, status, ": NULL status")) return why;
    return eq_bad_tasks(ev_task_cap(h->N, m, eq_lpt(m), 52 - 2 * h->N));
}

int pk_equity_ev_d(int device, int num_players, size_t m, const uint8_t *holes_d, const uint8_t *board_d, const uint8_t *nboard_d,
                   const uint16_t *live_d, const double *bets_d, uint64_t *share_d, uint8_t *level_seat_d, double *amount_d, double *ev_d,
                   uint32_t *boards_d, uint8_t *status_d, void *stream) {
    const char *call = "pk_equity_ev_d";
    EQ_REFUSE(g_fail, call, ev_check(num_players, m, holes_d && board_d && nboard_d && live_d && bets_d && status_d));
    const int N = num_players, lpt = eq_lpt(m);
    return eq_call_d(call, device, stream, m, EQ_TAB_EVAL, ev_layout(N, m, lpt, 50, !share_d, nullptr, nullptr), [&](hipStream_t st, const uint32_t *tab, char *work) {
        EvWork w;
        ev_layout(N, m, lpt, 50, !share_d, work, &w);
        const EqSpots spots{holes_d, board_d, nboard_d, live_d};
        return ev_launch(st, tab, &spots, bets_d, nullptr, N, m, EvOut{share_d, level_seat_d, amount_d, ev_d, boards_d, status_d}, w, lpt);
    });
}

int pk_equity_ev(int device, int num_players, size_t m, const uint8_t *holes, const uint8_t *board, const uint8_t *nboard, const uint16_t *live,
                 const double *bets, uint64_t *share, uint8_t *level_seat, double *amount, double *ev, uint32_t *boards, uint8_t *status) {
    const char *call = "pk_equity_ev";
    EQ_REFUSE(g_fail, call, ev_check(num_players, m, holes && board && nboard && live && bets && status));
    const int N = num_players, lpt = eq_lpt(m);
    Stage g;
    const int ho = g.in(holes, m * N * 2), bo = g.in(board, m * 5), nb = g.in(nboard, m), lv = g.in(live, m * 2), be = g.in(bets, m * N * 8);
    const EvStagedOut out(g, N, m, share, level_seat, amount, ev, boards, status);
    return eq_call_host(call, device, m, EQ_TAB_EVAL, g, ev_layout(N, m, lpt, 50, !share, nullptr, nullptr), [&](hipStream_t st, const uint32_t *tab, char *work) {
        EvWork w;
        ev_layout(N, m, lpt, 50, !share, work, &w);
        const EqSpots spots{g.at<uint8_t>(ho), g.at<uint8_t>(bo), g.at<uint8_t>(nb), g.at<uint16_t>(lv)};
        return ev_launch(st, tab, &spots, g.at<double>(be), nullptr, N, m, out.at(g), w, lpt);
    });
}

int pk_table_equity_ev_d(pk_handle *h, const int32_t *tables_d, size_t m, uint64_t *share_d, uint8_t *level_seat_d, double *amount_d, double *ev_d,
                         uint32_t *boards_d, uint8_t *status_d) {
    if (!h) return PK_E_INVALID_ARG;
    const char *call = "pk_table_equity_ev_d";
    EQ_REFUSE(h->fail, call, ev_table_check(h, m, status_d));
    const int N = h->N, lpt = eq_lpt(m), pool = 52 - 2 * N;
    return eq_table_call_d(h, call, tables_d, m, EQ_TAB_EVAL, ev_layout(N, m, lpt, pool, !share_d, nullptr, nullptr), [&](const uint32_t *tab, const EqTables &t, char *work) {
        EvWork w;
        ev_layout(N, m, lpt, pool, !share_d, work, &w);
        const EvTables et{t, h->S.bets, h->S.pending};     // (the handle's bets and pending chips beside the tables)
        return ev_launch(h->stream, tab, nullptr, nullptr, &et, N, m, EvOut{share_d, level_seat_d, amount_d, ev_d, boards_d, status_d}, w, lpt);
    });
}

int pk_table_equity_ev(pk_handle *h, const int32_t *tables, size_t m, uint64_t *share, uint8_t *level_seat, double *amount, double *ev,
                       uint32_t *boards, uint8_t *status) {
    if (!h) return PK_E_INVALID_ARG;
    const char *call = "pk_table_equity_ev";
    EQ_REFUSE(h->fail, call, ev_table_check(h, m, status));
    const int N = h->N, lpt = eq_lpt(m), pool = 52 - 2 * N;
    Stage g;
    const EvStagedOut out(g, N, m, share, level_seat, amount, ev, boards, status);
    return eq_table_call(h, call, tables, m, EQ_TAB_EVAL, g, ev_layout(N, m, lpt, pool, !share, nullptr, nullptr), [&](const uint32_t *tab, const EqTables &t, char *work) {
        EvWork w;
        ev_layout(N, m, lpt, pool, !share, work, &w);
        const EvTables et{t, h->S.bets, h->S.pending};
        return ev_launch(h->stream, tab, nullptr, nullptr, &et, N, m, out.at(g), w, lpt);
    });
}

// ---- sampled showdown equity (pokerl_hip.h "Sampled showdown equity"; kernels: pk_equity_sampled.hip).  Work space: the descriptors.
static EqsOut eqs_out(const EqOut &o) { return EqsOut{o.win, o.tie, o.share, o.boards, o.status}; }
static EqsStream eqs_seed_stream(uint64_t seed, uint32_t nonce, uint32_t samples, const uint32_t *ids) {
    return EqsStream{(uint32_t)seed, (uint32_t)(seed >> 32), nonce, samples, 0u, ids};
}
// The table forms draw with the handle's key, stream id = table_id_base + table
static EqsStream eqs_table_stream(const pk_handle *h, uint32_t nonce, uint32_t samples) {
    return EqsStream{h->S.key0, h->S.key1, nonce, samples, h->S.table_id_base, nullptr};
}
static const char *eqs_check(int num_players, size_t m, uint32_t samples, bool inputs) {
    if (const char *why = eq_bad_spots(num_players, m)) return why;
    if (const char *why = eqs_bad_samples(samples)) return why;
    if (const char *why = eq_null(m, inputs)) return why;
    return eqs_bad_tasks(m, samples);
}
static const char *eqs_table_check(const pk_handle *h, size_t m, int observer, uint32_t samples) {
    if (const char *why = eq_bad_m(m)) return why;
    if (const char *why = eqs_bad_samples(samples)) return why;
    if (const char *why = eqs_bad_observer(observer, h->N)) return why;
    return eqs_bad_tasks(m, samples);
}

int pk_equity_sampled_d(int device, int num_players, size_t m, const uint8_t *holes_d, const uint8_t *board_d, const uint8_t *nboard_d,
                        const uint16_t *live_d, const uint32_t *ids_d, uint32_t samples, uint64_t seed, uint32_t nonce, uint32_t *win_d,
                        uint32_t *tie_d, uint64_t *share_d, uint32_t *samples_d, uint8_t *status_d, void *stream) {
    const char *call = "pk_equity_sampled_d";
    EQ_REFUSE(g_fail, call, eqs_check(num_players, m, samples, holes_d && board_d && nboard_d && live_d));
    return eq_call_d(call, device, stream, m, EQ_TAB_EVAL, eqs_work_bytes(num_players, m), [&](hipStream_t st, const uint32_t *tab, char *work) {
        const EqSpots spots{holes_d, board_d, nboard_d, live_d};
        return eqs_launch(st, tab, &spots, nullptr, PK_OBSERVER_NONE, eqs_seed_stream(seed, nonce, samples, ids_d), num_players, m,
                          EqsOut{win_d, tie_d, share_d, samples_d, status_d}, (uint64_t *)work);
    });
}

int pk_equity_sampled(int device, int num_players, size_t m, const uint8_t *holes, const uint8_t *board, const uint8_t *nboard,
                      const uint16_t *live, const uint32_t *ids, uint32_t samples, uint64_t seed, uint32_t nonce, uint32_t *win, uint32_t *tie,
                      uint64_t *share, uint32_t *samples_out, uint8_t *status) {
    const char *call = "pk_equity_sampled";
    EQ_REFUSE(g_fail, call, eqs_check(num_players, m, samples, holes && board && nboard && live));
    const int N = num_players;
    Stage g;
    const int ho = g.in(holes, m * N * 2), bo = g.in(board, m * 5), nb = g.in(nboard, m), lv = g.in(live, m * 2), id = g.in(ids, m * 4);
    const EqStagedOut out(g, N, m, win, tie, share, samples_out, status);
    return eq_call_host(call, device, m, EQ_TAB_EVAL, g, eqs_work_bytes(N, m), [&](hipStream_t st, const uint32_t *tab, char *work) {
        const EqSpots spots{g.at<uint8_t>(ho), g.at<uint8_t>(bo), g.at<uint8_t>(nb), g.at<uint16_t>(lv)};
        return eqs_launch(st, tab, &spots, nullptr, PK_OBSERVER_NONE, eqs_seed_stream(seed, nonce, samples, g.at<uint32_t>(id)), N, m,
                          eqs_out(out.at(g)), (uint64_t *)work);
    });
}

// The table forms: the handle's own state as `observer` sees it
int pk_table_equity_sampled_d(pk_handle *h, const int32_t *tables_d, size_t m, int observer, uint32_t samples, uint32_t nonce, uint32_t *win_d,
                              uint32_t *tie_d, uint64_t *share_d, uint32_t *samples_d, uint8_t *status_d) {
    if (!h) return PK_E_INVALID_ARG;
    const char *call = "pk_table_equity_sampled_d";
    EQ_REFUSE(h->fail, call, eqs_table_check(h, m, observer, samples));
    return eq_table_call_d(h, call, tables_d, m, EQ_TAB_EVAL, eqs_work_bytes(h->N, m), [&](const uint32_t *tab, const EqTables &t, char *work) {
        return eqs_launch(h->stream, tab, nullptr, &t, observer, eqs_table_stream(h, nonce, samples), h->N, m,
                          EqsOut{win_d, tie_d, share_d, samples_d, status_d}, (uint64_t *)work);
    });
}

int pk_table_equity_sampled(pk_handle *h, const int32_t *tables, size_t m, int observer, uint32_t samples, uint32_t nonce, uint32_t *win,
                            uint32_t *tie, uint64_t *share, uint32_t *samples_out, uint8_t *status) {
    if (!h) return PK_E_INVALID_ARG;
    const char *call = "pk_table_equity_sampled";
    EQ_REFUSE(h->fail, call, eqs_table_check(h, m, observer, samples));
    Stage g;
    const EqStagedOut out(g, h->N, m, win, tie, share, samples_out, status);
    return eq_table_call(h, call, tables, m, EQ_TAB_EVAL, g, eqs_work_bytes(h->N, m), [&](const uint32_t *tab, const EqTables &t, char *work) {
        return eqs_launch(h->stream, tab, nullptr, &t, observer, eqs_table_stream(h, nonce, samples), h->N, m, eqs_out(out.at(g)), (uint64_t *)work);
    });
}

// ---- ranged sampled equity (pokerl_hip.h "Ranged sampled equity"; kernels: pk_equity_ranged.hip).  Work space: the cumulative sums of the
// call's range rows, then the descriptors.
static EqwOut eqw_out(const EqOut &o) { return EqwOut{o.win, o.tie, o.share, o.boards, o.status}; }
static const char *eqw_check(int num_players, size_t m, uint32_t samples, bool inputs, const uint16_t *weights, uint32_t num_ranges) {
    if (const char *why = eqs_check(num_players, m, samples, inputs)) return why;
    return eqw_bad_ranges(weights, num_ranges);
}
static const char *eqw_table_check(const pk_handle *h, size_t m, int observer, uint32_t samples, const uint16_t *weights, uint32_t num_ranges) {
    if (const char *why = eq_bad_m(m)) return why;
    if (const char *why = eqs_bad_samples(samples)) return why;
    if (const char *why = eqw_bad_observer(observer, h->N)) return why;
    if (const char *why = eqw_bad_ranges(weights, num_ranges)) return why;
    return eqs_bad_tasks(m, samples);
}

int pk_equity_ranged_d(int device, int num_players, size_t m, const uint8_t *holes_d, const uint8_t *board_d, const uint8_t *nboard_d,
                       const uint16_t *live_d, const uint32_t *ids_d, uint32_t samples, uint64_t seed, uint32_t nonce, const uint16_t *weights_d,
                       uint32_t num_ranges, const uint16_t *range_of_d, uint32_t *win_d, uint32_t *tie_d, uint64_t *share_d, uint32_t *accepted_d,
                       uint8_t *status_d, void *stream) {
    const char *call = "pk_equity_ranged_d";
    EQ_REFUSE(g_fail, call, eqw_check(num_players, m, samples, holes_d && board_d && nboard_d && live_d, weights_d, num_ranges));
    return eq_call_d(call, device, stream, m, EQ_TAB_EVAL, eqw_work_bytes(num_players, m, num_ranges), [&](hipStream_t st, const uint32_t *tab, char *work) {
        const EqSpots spots{holes_d, board_d, nboard_d, live_d};
        return eqw_launch(st, tab, &spots, nullptr, PK_OBSERVER_ACTIVE, eqs_seed_stream(seed, nonce, samples, ids_d),
                          EqwRanges{weights_d, num_ranges, range_of_d, 1}, num_players, m, EqwOut{win_d, tie_d, share_d, accepted_d, status_d}, work);
    });
}

int pk_equity_ranged(int device, int num_players, size_t m, const uint8_t *holes, const uint8_t *board, const uint8_t *nboard, const uint16_t *live,
                     const uint32_t *ids, uint32_t samples, uint64_t seed, uint32_t nonce, const uint16_t *weights, uint32_t num_ranges,
                     const uint16_t *range_of, uint32_t *win, uint32_t *tie, uint64_t *share, uint32_t *accepted, uint8_t *status) {
    const char *call = "pk_equity_ranged";
    EQ_REFUSE(g_fail, call, eqw_check(num_players, m, samples, holes && board && nboard && live, weights, num_ranges));
    const int N = num_players;
    Stage g;
    const int ho = g.in(holes, m * N * 2), bo = g.in(board, m * 5), nb = g.in(nboard, m), lv = g.in(live, m * 2), id = g.in(ids, m * 4);
    const int wt = g.in(num_ranges ? weights : nullptr, (size_t)num_ranges * EQW_HOLDINGS * 2), ro = g.in(range_of, m * (size_t)N * 2);
    const EqStagedOut out(g, N, m, win, tie, share, accepted, status);
    return eq_call_host(call, device, m, EQ_TAB_EVAL, g, eqw_work_bytes(N, m, num_ranges), [&](hipStream_t st, const uint32_t *tab, char *work) {
        const EqSpots spots{g.at<uint8_t>(ho), g.at<uint8_t>(bo), g.at<uint8_t>(nb), g.at<uint16_t>(lv)};
        return eqw_launch(st, tab, &spots, nullptr, PK_OBSERVER_ACTIVE, eqs_seed_stream(seed, nonce, samples, g.at<uint32_t>(id)),
                          EqwRanges{g.at<uint16_t>(wt), num_ranges, g.at<uint16_t>(ro), 1}, N, m, eqw_out(out.at(g)), work);
    });
}

// The table forms: the handle's own state as `observer` sees it
int pk_table_equity_ranged_d(pk_handle *h, const int32_t *tables_d, size_t m, int observer, uint32_t samples, uint32_t nonce, const uint16_t *weights_d,
                             uint32_t num_ranges, const uint16_t *range_of_d, int range_per_table, uint32_t *win_d, uint32_t *tie_d, uint64_t *share_d,
                             uint32_t *accepted_d, uint8_t *status_d) {
    if (!h) return PK_E_INVALID_ARG;
    const char *call = "pk_table_equity_ranged_d";
    EQ_REFUSE(h->fail, call, eqw_table_check(h, m, observer, samples, weights_d, num_ranges));
    return eq_table_call_d(h, call, tables_d, m, EQ_TAB_EVAL, eqw_work_bytes(h->N, m, num_ranges), [&](const uint32_t *tab, const EqTables &t, char *work) {
        return eqw_launch(h->stream, tab, nullptr, &t, observer, eqs_table_stream(h, nonce, samples),
                          EqwRanges{weights_d, num_ranges, range_of_d, range_per_table ? 1 : 0}, h->N, m,
                          EqwOut{win_d, tie_d, share_d, accepted_d, status_d}, work);
    });
}

int pk_table_equity_ranged(pk_handle *h, const int32_t *tables, size_t m, int observer, uint32_t samples, uint32_t nonce, const uint16_t *weights,
                           uint32_t num_ranges, const uint16_t *range_of, int range_per_table, uint32_t *win, uint32_t *tie, uint64_t *share,
                           uint32_t *accepted, uint8_t *status) {
    if (!h) return PK_E_INVALID_ARG;
    const char *call = "pk_table_equity_ranged";
    EQ_REFUSE(h->fail, call, eqw_table_check(h, m, observer, samples, weights, num_ranges));
    Stage g;
    const int wt = g.in(num_ranges ? weights : nullptr, (size_t)num_ranges * EQW_HOLDINGS * 2);
    const int ro = g.in(range_of, (range_per_table ? m : (size_t)1) * (size_t)h->N * 2);
    const EqStagedOut out(g, h->N, m, win, tie, share, accepted, status);
    return eq_table_call(h, call, tables, m, EQ_TAB_EVAL, g, eqw_work_bytes(h->N, m, num_ranges), [&](const uint32_t *tab, const EqTables &t, char *work) {
        return eqw_launch(h->stream, tab, nullptr, &t, observer, eqs_table_stream(h, nonce, samples),
                          EqwRanges{g.at<uint16_t>(wt), num_ranges, g.at<uint16_t>(ro), range_per_table ? 1 : 0}, h->N, m, eqw_out(out.at(g)), work);
    });
}

// ---- ranged showdown EV in chips (pokerl_hip.h "Ranged showdown EV"; kernels: pk_ev_ranged.hip).  Work space: the ranged family's (cumulative
// sums, descriptors), then the level table, the bets, the amounts and -- when the caller does not ask for them -- `share` and `accepted`.
struct EvwStagedOut {
    int share, level_seat, amount, ev, accepted, status;
    EvwStagedOut(Stage &g, int N, size_t m, uint64_t *share, uint8_t *level_seat, double *amount, double *ev, uint32_t *accepted, uint8_t *status)
        : share(g.out(share, m * N * N * 8)), level_seat(g.out(level_seat, m * N)), amount(g.out(amount, m * N * 8)), ev(g.out(ev, m * N * 8)),
          accepted(g.out(accepted, m * 4)), status(g.out(status, m)) {}
    EvwOut at(const Stage &g) const {
        return EvwOut{g.at<uint64_t>(share), g.at<uint8_t>(level_seat), g.at<double>(amount), g.at<double>(ev), g.at<uint32_t>(accepted), g.at<uint8_t>(status)};
    }
};
static const char *evw_bad_tasks(int N, size_t m, uint32_t samples) {
    return evw_task_bound(N, m, samples) > EQ_TASKS_MAX ? ": m * ceil(samples / 64) * (groups of levels) must fit 32 bits: split the batch" : nullptr;
}
static const char *evw_check(int num_players, size_t m, uint32_t samples, bool inputs_and_status, const uint16_t *weights, uint32_t num_ranges) {
    if (const char *why = eq_bad_spots(num_players, m)) return why;
    if (const char *why = eqs_bad_samples(samples)) return why;
    if (const char *why = eqw_bad_ranges(weights, num_ranges)) return why;
    if (const char *why = eq_null(m, inputs_and_status, ": NULL input buffer or NULL status")) return why;
    return evw_bad_tasks(num_players, m, samples);
}
static const char *evw_table_check(const pk_handle *h, size_t m, int observer, uint32_t samples, const uint16_t *weights, uint32_t num_ranges,
                                   const uint8_t *status) {
    if (const char *why = eq_bad_m(m)) return why;
    if (const char *why = eqs_bad_samples(samples)) return why;
    if (const char *why = eqw_bad_observer(observer, h->N)) return why;
    if (const char *why = eqw_bad_ranges(weights, num_ranges)) return why;
    if (const char *why = eq_null(m, status, ": NULL status")) return why;
    return evw_bad_tasks(h->N, m, samples);
}

int pk_ev_ranged_d(int device, int num_players, size_t m, const uint8_t *holes_d, const uint8_t *board_d, const uint8_t *nboard_d,
                   const uint16_t *live_d, const double *bets_d, const uint32_t *ids_d, uint32_t samples, uint64_t seed, uint32_t nonce,
                   const uint16_t *weights_d, uint32_t num_ranges, const uint16_t *range_of_d, uint64_t *share_d, uint8_t *level_seat_d,
                   double *amount_d, double *ev_d, uint32_t *accepted_d, uint8_t *status_d, void *stream) {
    const char *call = "pk_ev_ranged_d";
    EQ_REFUSE(g_fail, call, evw_check(num_players, m, samples, holes_d && board_d && nboard_d && live_d && bets_d && status_d, weights_d, num_ranges));
    const int N = num_players;
    return eq_call_d(call, device, stream, m, EQ_TAB_EVAL, evw_layout(N, m, num_ranges, !share_d, !accepted_d, nullptr, nullptr), [&](hipStream_t st, const uint32_t *tab, char *work) {
        EvwWork w;
        evw_layout(N, m, num_ranges, !share_d, !accepted_d, work, &w);
        const EqSpots spots{holes_d, board_d, nboard_d, live_d};
        return evw_launch(st, tab, &spots, bets_d, nullptr, PK_OBSERVER_ACTIVE, eqs_seed_stream(seed, nonce, samples, ids_d),
                          EqwRanges{weights_d, num_ranges, range_of_d, 1}, N, m, EvwOut{share_d, level_seat_d, amount_d, ev_d, accepted_d, status_d}, w);
    });
}

int pk_ev_ranged(int device, int num_players, size_t m, const uint8_t *holes, const uint8_t *board, const uint8_t *nboard, const uint16_t *live,
                 const double *bets, const uint32_t *ids, uint32_t samples, uint64_t seed, uint32_t nonce, const uint16_t *weights,
                 uint32_t num_ranges, const uint16_t *range_of, uint64_t *share, uint8_t *level_seat, double *amount, double *ev, uint32_t *accepted,
                 uint8_t *status) {
    const char *call = "pk_ev_ranged";
    EQ_REFUSE(g_fail, call, evw_check(num_players, m, samples, holes && board && nboard && live && bets && status, weights, num_ranges));
    const int N = num_players;
    Stage g;
    const int ho = g.in(holes, m * N * 2), bo = g.in(board, m * 5), nb = g.in(nboard, m), lv = g.in(live, m * 2), be = g.in(bets, m * N * 8), id = g.in(ids, m * 4);
    const int wt = g.in(num_ranges ? weights : nullptr, (size_t)num_ranges * EQW_HOLDINGS * 2), ro = g.in(range_of, m * (size_t)N * 2);
    const EvwStagedOut out(g, N, m, share, level_seat, amount, ev, accepted, status);
    return eq_call_host(call, device, m, EQ_TAB_EVAL, g, evw_layout(N, m, num_ranges, !share, !accepted, nullptr, nullptr), [&](hipStream_t st, const uint32_t *tab, char *work) {
        EvwWork w;
        evw_layout(N, m, num_ranges, !share, !accepted, work, &w);
        const EqSpots spots{g.at<uint8_t>(ho), g.at<uint8_t>(bo), g.at<uint8_t>(nb), g.at<uint16_t>(lv)};
        return evw_launch(st, tab, &spots, g.at<double>(be), nullptr, PK_OBSERVER_ACTIVE, eqs_seed_stream(seed, nonce, samples, g.at<uint32_t>(id)),
                          EqwRanges{g.at<uint16_t>(wt), num_ranges, g.at<uint16_t>(ro), 1}, N, m, out.at(g), w);
    });
}

// The table forms: the handle's own state as `observer` sees it, bets = bets + pending_bets
int pk_table_ev_ranged_d(pk_handle *h, const int32_t *tables_d, size_t m, int observer, uint32_t samples, uint32_t nonce, const uint16_t *weights_d,
                         uint32_t num_ranges, const uint16_t *range_of_d, int range_per_table, uint64_t *share_d, uint8_t *level_seat_d,
                         double *amount_d, double *ev_d, uint32_t *accepted_d, uint8_t *status_d) {
    if (!h) return PK_E_INVALID_ARG;
    const char *call = "pk_table_ev_ranged_d";
    EQ_REFUSE(h->fail, call, evw_table_check(h, m, observer, samples, weights_d, num_ranges, status_d));
    const int N = h->N;
    return eq_table_call_d(h, call, tables_d, m, EQ_TAB_EVAL, evw_layout(N, m, num_ranges, !share_d, !accepted_d, nullptr, nullptr), [&](const uint32_t *tab, const EqTables &t, char *work) {
        EvwWork w;
        evw_layout(N, m, num_ranges, !share_d, !accepted_d, work, &w);
        const EvTables et{t, h->S.bets, h->S.pending};     // (the handle's bets and pending chips beside the tables)
        return evw_launch(h->stream, tab, nullptr, nullptr, &et, observer, eqs_table_stream(h, nonce, samples),
                          EqwRanges{weights_d, num_ranges, range_of_d, range_per_table ? 1 : 0}, N, m,
                          EvwOut{share_d, level_seat_d, amount_d, ev_d, accepted_d, status_d}, w);
    });
}

int pk_table_ev_ranged(pk_handle *h, const int32_t *tables, size_t m, int observer, uint32_t samples, uint32_t nonce, const uint16_t *weights,
                       uint32_t num_ranges, const uint16_t *range_of, int range_per_table, uint64_t *share, uint8_t *level_seat, double *amount,
                       double *ev, uint32_t *accepted, uint8_t *status) {
    if (!h) return PK_E_INVALID_ARG;
    const char *call = "pk_table_ev_ranged";
    EQ_REFUSE(h->fail, call, evw_table_check(h, m, observer, samples, weights, num_ranges, status));
    const int N = h->N;
    Stage g;
    const int wt = g.in(num_ranges ? weights : nullptr, (size_t)num_ranges * EQW_HOLDINGS * 2);
    const int ro = g.in(range_of, (range_per_table ? m : (size_t)1) * (size_t)N * 2);
    const EvwStagedOut out(g, N, m, share, level_seat, amount, ev, accepted, status);
    return eq_table_call(h, call, tables, m, EQ_TAB_EVAL, g, evw_layout(N, m, num_ranges, !share, !accepted, nullptr, nullptr), [&](const uint32_t *tab, const EqTables &t, char *work) {
        EvwWork w;
        evw_layout(N, m, num_ranges, !share, !accepted, work, &w);
        const EvTables et{t, h->S.bets, h->S.pending};
        return evw_launch(h->stream, tab, nullptr, nullptr, &et, observer, eqs_table_stream(h, nonce, samples),
                          EqwRanges{g.at<uint16_t>(wt), num_ranges, g.at<uint16_t>(ro), range_per_table ? 1 : 0}, N, m, out.at(g), w);
    });
}

// ---- range equity (pokerl_hip.h "Range equity"; kernels: pk_equity_range.hip).  Work space: the descriptors.
static size_t eqr_weight_bytes(size_t m, int per_spot) { return (per_spot ? m : (size_t)1) * EQR_HOLDINGS * 2; }
static const char *eqr_check(size_t m, bool inputs) {   // (range equity, range vs range and the histograms: no seat count, no task list)
    if (const char *why = eq_bad_m(m)) return why;
    return eq_null(m, inputs);
}
static const char *eqr_table_check(const pk_handle *h, size_t m, int observer) {
    if (const char *why = eq_bad_m(m)) return why;
    return eqr_bad_observer(observer, h->N);
}

int pk_equity_range_d(int device, size_t m, const uint8_t *hero_d, const uint8_t *board_d, const uint8_t *nboard_d, const uint64_t *dead_d,
                      const uint16_t *weights_d, int weights_per_spot, uint64_t *agg_d, uint32_t *win_d, uint32_t *tie_d, uint32_t *boards_d,
                      uint8_t *status_d, void *stream) {
    const char *call = "pk_equity_range_d";
    EQ_REFUSE(g_fail, call, eqr_check(m, hero_d && board_d && nboard_d));
    return eq_call_d(call, device, stream, m, EQ_TAB_EVAL, eqr_work_bytes(m), [&](hipStream_t st, const uint32_t *tab, char *work) {
        const EqrSpots spots{hero_d, board_d, nboard_d, dead_d};
        return eqr_launch(st, tab, &spots, nullptr, 0, PK_OBSERVER_NONE, EqrWeights{weights_d, weights_per_spot != 0}, m,
                          EqrOut{agg_d, win_d, tie_d, boards_d, status_d}, (uint64_t *)work);
    });
}

int pk_equity_range(int device, size_t m, const uint8_t *hero, const uint8_t *board, const uint8_t *nboard, const uint64_t *dead,
                    const uint16_t *weights, int weights_per_spot, uint64_t *agg, uint32_t *win, uint32_t *tie, uint32_t *boards,
                    uint8_t *status) {
    const char *call = "pk_equity_range";
    EQ_REFUSE(g_fail, call, eqr_check(m, hero && board && nboard));
    Stage g;
    const int he = g.in(hero, m * 2), bo = g.in(board, m * 5), nb = g.in(nboard, m), de = g.in(dead, m * 8);
    const int we = g.in(weights, eqr_weight_bytes(m, weights_per_spot));
    const EqrStagedOut out(g, m, agg, win, tie, boards, status);
    return eq_call_host(call, device, m, EQ_TAB_EVAL, g, eqr_work_bytes(m), [&](hipStream_t st, const uint32_t *tab, char *work) {
        const EqrSpots spots{g.at<uint8_t>(he), g.at<uint8_t>(bo), g.at<uint8_t>(nb), g.at<uint64_t>(de)};
        return eqr_launch(st, tab, &spots, nullptr, 0, PK_OBSERVER_NONE, EqrWeights{g.at<uint16_t>(we), weights_per_spot != 0}, m, out.at(g),
                          (uint64_t *)work);
    });
}

// The table forms: the handle's own state as `observer` sees it
int pk_table_equity_range_d(pk_handle *h, const int32_t *tables_d, size_t m, int observer, const uint16_t *weights_d, int weights_per_spot,
                            uint64_t *agg_d, uint32_t *win_d, uint32_t *tie_d, uint32_t *boards_d, uint8_t *status_d) {
    if (!h) return PK_E_INVALID_ARG;
    const char *call = "pk_table_equity_range_d";
    EQ_REFUSE(h->fail, call, eqr_table_check(h, m, observer));
    return eq_table_call_d(h, call, tables_d, m, EQ_TAB_EVAL, eqr_work_bytes(m), [&](const uint32_t *tab, const EqTables &t, char *work) {
        return eqr_launch(h->stream, tab, nullptr, &t, h->N, observer, EqrWeights{weights_d, weights_per_spot != 0}, m,
                          EqrOut{agg_d, win_d, tie_d, boards_d, status_d}, (uint64_t *)work);
    });
}

int pk_table_equity_range(pk_handle *h, const int32_t *tables, size_t m, int observer, const uint16_t *weights, int weights_per_spot,
                          uint64_t *agg, uint32_t *win, uint32_t *tie, uint32_t *boards, uint8_t *status) {
    if (!h) return PK_E_INVALID_ARG;
    const char *call = "pk_table_equity_range";
    EQ_REFUSE(h->fail, call, eqr_table_check(h, m, observer));
    Stage g;
    const int we = g.in(weights, eqr_weight_bytes(m, weights_per_spot));
    const EqrStagedOut out(g, m, agg, win, tie, boards, status);
    return eq_table_call(h, call, tables, m, EQ_TAB_EVAL, g, eqr_work_bytes(m), [&](const uint32_t *tab, const EqTables &t, char *work) {
        return eqr_launch(h->stream, tab, nullptr, &t, h->N, observer, EqrWeights{g.at<uint16_t>(we), weights_per_spot != 0}, m, out.at(g), (uint64_t *)work);
    });
}

// ---- range against range (pokerl_hip.h "Range vs range"; kernels: pk_equity_rvr.hip).  Work space: the descriptors.  The table forms read
// the public board of the handle's own tables (no hole card is read: there is no observer).
int pk_equity_rvr_d(int device, size_t m, const uint8_t *board_d, const uint8_t *nboard_d, const uint64_t *dead_d, const uint16_t *weights_d,
                    int weights_per_spot, uint64_t *win_d, uint64_t *tie_d, uint64_t *tot_d, uint32_t *boards_d, uint8_t *status_d, void *stream) {
    const char *call = "pk_equity_rvr_d";
    EQ_REFUSE(g_fail, call, eqr_check(m, board_d && nboard_d));
    return eq_call_d(call, device, stream, m, EQ_TAB_EVAL, rvr_work_bytes(m), [&](hipStream_t st, const uint32_t *tab, char *work) {
        const RvrSpots spots{board_d, nboard_d, dead_d};
        return rvr_launch(st, tab, &spots, nullptr, RvrWeights{weights_d, weights_per_spot != 0}, m, RvrOut{win_d, tie_d, tot_d, boards_d, status_d},
                          (uint64_t *)work);
    });
}

int pk_equity_rvr(int device, size_t m, const uint8_t *board, const uint8_t *nboard, const uint64_t *dead, const uint16_t *weights,
                  int weights_per_spot, uint64_t *win, uint64_t *tie, uint64_t *tot, uint32_t *boards, uint8_t *status) {
    const char *call = "pk_equity_rvr";
    EQ_REFUSE(g_fail, call, eqr_check(m, board && nboard));
    Stage g;
    const int bo = g.in(board, m * 5), nb = g.in(nboard, m), de = g.in(dead, m * 8);
    const int we = g.in(weights, eqr_weight_bytes(m, weights_per_spot));
    const RvrStagedOut out(g, m, win, tie, tot, boards, status);
    return eq_call_host(call, device, m, EQ_TAB_EVAL, g, rvr_work_bytes(m), [&](hipStream_t st, const uint32_t *tab, char *work) {
        const RvrSpots spots{g.at<uint8_t>(bo), g.at<uint8_t>(nb), g.at<uint64_t>(de)};
        return rvr_launch(st, tab, &spots, nullptr, RvrWeights{g.at<uint16_t>(we), weights_per_spot != 0}, m, out.at(g), (uint64_t *)work);
    });
}

int pk_table_equity_rvr_d(pk_handle *h, const int32_t *tables_d, size_t m, const uint16_t *weights_d, int weights_per_spot, uint64_t *win_d,
                          uint64_t *tie_d, uint64_t *tot_d, uint32_t *boards_d, uint8_t *status_d) {
    if (!h) return PK_E_INVALID_ARG;
    const char *call = "pk_table_equity_rvr_d";
    EQ_REFUSE(h->fail, call, eq_bad_m(m));
    return eq_table_call_d(h, call, tables_d, m, EQ_TAB_EVAL, rvr_work_bytes(m), [&](const uint32_t *tab, const EqTables &t, char *work) {
        return rvr_launch(h->stream, tab, nullptr, &t, RvrWeights{weights_d, weights_per_spot != 0}, m, RvrOut{win_d, tie_d, tot_d, boards_d, status_d},
                          (uint64_t *)work);
    });
}

int pk_table_equity_rvr(pk_handle *h, const int32_t *tables, size_t m, const uint16_t *weights, int weights_per_spot, uint64_t *win, uint64_t *tie,
                        uint64_t *tot, uint32_t *boards, uint8_t *status) {
    if (!h) return PK_E_INVALID_ARG;
    const char *call = "pk_table_equity_rvr";
    EQ_REFUSE(h->fail, call, eq_bad_m(m));
    Stage g;
    const int we = g.in(weights, eqr_weight_bytes(m, weights_per_spot));
    const RvrStagedOut out(g, m, win, tie, tot, boards, status);
    return eq_table_call(h, call, tables, m, EQ_TAB_EVAL, g, rvr_work_bytes(m), [&](const uint32_t *tab, const EqTables &t, char *work) {
        return rvr_launch(h->stream, tab, nullptr, &t, RvrWeights{g.at<uint16_t>(we), weights_per_spot != 0}, m, out.at(g), (uint64_t *)work);
    });
}

// ---- strength histograms (pokerl_hip.h "Strength histograms"; kernels: pk_equity_hist.hip).  Spots, weights and work space as range vs range.
static_assert(HIST_MAX_BINS == PK_EQ_HIST_MAX_BINS, "pk_equity_hist.hpp and the ABI header agree");
static const char *hist_check(size_t m, bool inputs, int nbins) {
    if (const char *why = eqr_check(m, inputs)) return why;
    return hist_bad_bins(nbins);
}
static const char *hist_table_check(size_t m, int nbins) {
    if (const char *why = eq_bad_m(m)) return why;
    return hist_bad_bins(nbins);
}

int pk_equity_hist_d(int device, size_t m, const uint8_t *board_d, const uint8_t *nboard_d, const uint64_t *dead_d, const uint16_t *weights_d,
                     int weights_per_spot, int nbins, uint16_t *hist_d, uint16_t *void_d, uint32_t *completions_d, uint8_t *status_d, void *stream) {
    const char *call = "pk_equity_hist_d";
    EQ_REFUSE(g_fail, call, hist_check(m, board_d && nboard_d, nbins));
    return eq_call_d(call, device, stream, m, EQ_TAB_EVAL, rvr_work_bytes(m), [&](hipStream_t st, const uint32_t *tab, char *work) {
        const RvrSpots spots{board_d, nboard_d, dead_d};
        return hist_launch(st, tab, &spots, nullptr, RvrWeights{weights_d, weights_per_spot != 0}, m, nbins,
                           HistOut{hist_d, void_d, completions_d, status_d}, (uint64_t *)work);
    });
}

int pk_equity_hist(int device, size_t m, const uint8_t *board, const uint8_t *nboard, const uint64_t *dead, const uint16_t *weights,
                   int weights_per_spot, int nbins, uint16_t *hist, uint16_t *void_, uint32_t *completions, uint8_t *status) {
    const char *call = "pk_equity_hist";
    EQ_REFUSE(g_fail, call, hist_check(m, board && nboard, nbins));
    Stage g;
    const int bo = g.in(board, m * 5), nb = g.in(nboard, m), de = g.in(dead, m * 8);
    const int we = g.in(weights, eqr_weight_bytes(m, weights_per_spot));
    const HistStagedOut out(g, m, nbins, hist, void_, completions, status);
    return eq_call_host(call, device, m, EQ_TAB_EVAL, g, rvr_work_bytes(m), [&](hipStream_t st, const uint32_t *tab, char *work) {
        const RvrSpots spots{g.at<uint8_t>(bo), g.at<uint8_t>(nb), g.at<uint64_t>(de)};
        return hist_launch(st, tab, &spots, nullptr, RvrWeights{g.at<uint16_t>(we), weights_per_spot != 0}, m, nbins, out.at(g), (uint64_t *)work);
    });
}

int pk_table_equity_hist_d(pk_handle *h, const int32_t *tables_d, size_t m, const uint16_t *weights_d, int weights_per_spot, int nbins,
                           uint16_t *hist_d, uint16_t *void_d, uint32_t *completions_d, uint8_t *status_d) {
    if (!h) return PK_E_INVALID_ARG;
    const char *call = "pk_table_equity_hist_d";
    EQ_REFUSE(h->fail, call, hist_table_check(m, nbins));
    return eq_table_call_d(h, call, tables_d, m, EQ_TAB_EVAL, rvr_work_bytes(m), [&](const uint32_t *tab, const EqTables &t, char *work) {
        return hist_launch(h->stream, tab, nullptr, &t, RvrWeights{weights_d, weights_per_spot != 0}, m, nbins,
                           HistOut{hist_d, void_d, completions_d, status_d}, (uint64_t *)work);
    });
}

int pk_table_equity_hist(pk_handle *h, const int32_t *tables, size_t m, const uint16_t *weights, int weights_per_spot, int nbins, uint16_t *hist,
                         uint16_t *void_, uint32_t *completions, uint8_t *status) {
    if (!h) return PK_E_INVALID_ARG;
    const char *call = "pk_table_equity_hist";
    EQ_REFUSE(h->fail, call, hist_table_check(m, nbins));
    Stage g;
    const int we = g.in(weights, eqr_weight_bytes(m, weights_per_spot));
    const HistStagedOut out(g, m, nbins, hist, void_, completions, status);
    return eq_table_call(h, call, tables, m, EQ_TAB_EVAL, g, rvr_work_bytes(m), [&](const uint32_t *tab, const EqTables &t, char *work) {
        return hist_launch(h->stream, tab, nullptr, &t, RvrWeights{g.at<uint16_t>(we), weights_per_spot != 0}, m, nbins, out.at(g), (uint64_t *)work);
    });
}

// ---- hero strength histogram (pokerl_hip.h "Hero strength histogram"; kernels: pk_equity_hist_hero.hip).  Spots, weights and observer as range
// equity; the optional bucket stage is the clustering family's assign on the rows of the call.  Work space: pk::hh_work_bytes.
static_assert(HH_MAX_BINS == PK_EQ_HIST_MAX_BINS, "pk_equity_hist_hero.hpp and the ABI header agree");
static const char *hh_bad_bucket(int K, const void *centroids, const void *label, const void *dist) {
    if (K < 0 || K > PK_CL_MAX_K) return ": K must be 0 (no bucket stage) or 1 .. PK_CL_MAX_K (4096)";
    if (K > 0 && !centroids) return ": NULL centroids with K > 0";
    return K == 0 && (label || dist) ? ": label / dist asked for with K = 0 (no centroids to measure against)" : nullptr;
}
static const char *hh_check(size_t m, bool inputs, int nbins, int K, const void *centroids, const void *label, const void *dist) {
    if (const char *why = eqr_check(m, inputs)) return why;
    if (const char *why = hist_bad_bins(nbins)) return why;
    return hh_bad_bucket(K, centroids, label, dist);
}
static const char *hh_table_check(const pk_handle *h, size_t m, int observer, int nbins, int K, const void *centroids, const void *label, const void *dist) {
    if (const char *why = eqr_table_check(h, m, observer)) return why;
    if (const char *why = hist_bad_bins(nbins)) return why;
    return hh_bad_bucket(K, centroids, label, dist);
}

int pk_equity_hist_hero_d(int device, size_t m, const uint8_t *hero_d, const uint8_t *board_d, const uint8_t *nboard_d, const uint64_t *dead_d,
                          const uint16_t *weights_d, int weights_per_spot, int nbins, uint16_t *hist_d, uint16_t *void_d, uint32_t *completions_d,
                          uint8_t *status_d, int K, const uint16_t *centroids_d, uint16_t *label_d, uint32_t *dist_d, void *stream) {
    const char *call = "pk_equity_hist_hero_d";
    EQ_REFUSE(g_fail, call, hh_check(m, hero_d && board_d && nboard_d, nbins, K, centroids_d, label_d, dist_d));
    const HeroHistOut out{hist_d, void_d, completions_d, status_d};
    const HeroHistBucket bk{K, centroids_d, label_d, dist_d};
    return eq_call_d(call, device, stream, m, EQ_TAB_EVAL, hh_work_bytes(m, nbins, out, bk), [&](hipStream_t st, const uint32_t *tab, char *work) {
        const EqrSpots spots{hero_d, board_d, nboard_d, dead_d};
        return hh_launch(st, tab, &spots, nullptr, 0, PK_OBSERVER_NONE, EqrWeights{weights_d, weights_per_spot != 0}, m, nbins, out, bk, work);
    });
}

int pk_equity_hist_hero(int device, size_t m, const uint8_t *hero, const uint8_t *board, const uint8_t *nboard, const uint64_t *dead,
                        const uint16_t *weights, int weights_per_spot, int nbins, uint16_t *hist, uint16_t *void_, uint32_t *completions,
                        uint8_t *status, int K, const uint16_t *centroids, uint16_t *label, uint32_t *dist) {
    const char *call = "pk_equity_hist_hero";
    EQ_REFUSE(g_fail, call, hh_check(m, hero && board && nboard, nbins, K, centroids, label, dist));
    Stage g;
    const int he = g.in(hero, m * 2), bo = g.in(board, m * 5), nb = g.in(nboard, m), de = g.in(dead, m * 8);
    const int we = g.in(weights, eqr_weight_bytes(m, weights_per_spot));
    const HeroHistStaged io(g, m, nbins, hist, void_, completions, status, K, centroids, label, dist);
    const size_t bytes = hh_work_bytes(m, nbins, HeroHistOut{hist, void_, completions, status}, HeroHistBucket{K, centroids, label, dist});
    return eq_call_host(call, device, m, EQ_TAB_EVAL, g, bytes, [&](hipStream_t st, const uint32_t *tab, char *work) {
        const EqrSpots spots{g.at<uint8_t>(he), g.at<uint8_t>(bo), g.at<uint8_t>(nb), g.at<uint64_t>(de)};
        return hh_launch(st, tab, &spots, nullptr, 0, PK_OBSERVER_NONE, EqrWeights{g.at<uint16_t>(we), weights_per_spot != 0}, m, nbins, io.at(g),
                         io.bucket(g), work);
    });
}

// The table forms: the handle's own state as `observer` sees it
int pk_table_equity_hist_hero_d(pk_handle *h, const int32_t *tables_d, size_t m, int observer, const uint16_t *weights_d, int weights_per_spot, int nbins,
                                uint16_t *hist_d, uint16_t *void_d, uint32_t *completions_d, uint8_t *status_d, int K, const uint16_t *centroids_d,
                                uint16_t *label_d, uint32_t *dist_d) {
    if (!h) return PK_E_INVALID_ARG;
    const char *call = "pk_table_equity_hist_hero_d";
    EQ_REFUSE(h->fail, call, hh_table_check(h, m, observer, nbins, K, centroids_d, label_d, dist_d));
    const HeroHistOut out{hist_d, void_d, completions_d, status_d};
    const HeroHistBucket bk{K, centroids_d, label_d, dist_d};
    return eq_table_call_d(h, call, tables_d, m, EQ_TAB_EVAL, hh_work_bytes(m, nbins, out, bk), [&](const uint32_t *tab, const EqTables &t, char *work) {
        return hh_launch(h->stream, tab, nullptr, &t, h->N, observer, EqrWeights{weights_d, weights_per_spot != 0}, m, nbins, out, bk, work);
    });
}

int pk_table_equity_hist_hero(pk_handle *h, const int32_t *tables, size_t m, int observer, const uint16_t *weights, int weights_per_spot, int nbins,
                              uint16_t *hist, uint16_t *void_, uint32_t *completions, uint8_t *status, int K, const uint16_t *centroids, uint16_t *label,
                              uint32_t *dist) {
    if (!h) return PK_E_INVALID_ARG;
    const char *call = "pk_table_equity_hist_hero";
    EQ_REFUSE(h->fail, call, hh_table_check(h, m, observer, nbins, K, centroids, label, dist));
    Stage g;
    const int we = g.in(weights, eqr_weight_bytes(m, weights_per_spot));
    const HeroHistStaged io(g, m, nbins, hist, void_, completions, status, K, centroids, label, dist);
    const size_t bytes = hh_work_bytes(m, nbins, HeroHistOut{hist, void_, completions, status}, HeroHistBucket{K, centroids, label, dist});
    return eq_table_call(h, call, tables, m, EQ_TAB_EVAL, g, bytes, [&](const uint32_t *tab, const EqTables &t, char *work) {
        return hh_launch(h->stream, tab, nullptr, &t, h->N, observer, EqrWeights{g.at<uint16_t>(we), weights_per_spot != 0}, m, nbins, io.at(g), io.bucket(g),
                         work);
    });
}

// ---- histogram clustering (pokerl_hip.h "Histogram clustering"; kernels: pk_hist_cluster.hip).  The device and the host form of the family
// (n >= 1 rows stand where the spots do), no evaluator table.
static_assert(CL_MAX_K == PK_CL_MAX_K && CL_NONE == PK_CL_NONE && CL_MAX_BINS == PK_EQ_HIST_MAX_BINS, "pk_hist_cluster.hpp and the ABI header agree");
static const char *cl_check(size_t n, int nbins, int K, bool arrays) {
    if (const char *why = hist_bad_bins(nbins)) return why;
    if (n < 1 || n >= EQ_MAX_SPOTS) return ": n must be 1 .. 2^31 - 1";
    if (K < 1 || K > PK_CL_MAX_K) return ": K must be 1 .. PK_CL_MAX_K (4096)";
    return arrays ? nullptr : ": NULL array";
}
// seeding and clustering take their centroids from rows: K rows at least (assign labels any number of rows with any K)
static const char *cl_bad_k_rows(size_t n, int K) { return (size_t)K > n ? ": K is larger than the number of rows" : nullptr; }
static const char *cl_bad_iters(int iters) { return iters < 1 || iters > CL_MAX_ITERS ? ": iters must be 1 .. 1024" : nullptr; }
// the host forms see the rows: K non-empty ones at least
static const char *cl_bad_rows(size_t n, int nbins, const uint16_t *hist, int K) {
    size_t live = 0;
    for (size_t i = 0; i < n && live < (size_t)K; ++i) {
        uint32_t mass = 0;
        for (int b = 0; b < nbins; ++b) mass += hist[i * (size_t)nbins + b];
        live += mass != 0;
    }
    return live < (size_t)K ? ": K is larger than the number of non-empty rows" : nullptr;
}

int pk_hist_cluster_seed_d(int device, size_t n, int nbins, const uint16_t *hist_d, int K, uint64_t seed, uint32_t nonce, uint16_t *centroids_d,
                           void *stream) {
    const char *call = "pk_hist_cluster_seed_d";
    EQ_REFUSE(g_fail, call, cl_check(n, nbins, K, hist_d && centroids_d));
    EQ_REFUSE(g_fail, call, cl_bad_k_rows(n, K));
    return eq_call_d(call, device, stream, n, EQ_TAB_NONE, cl_work_bytes(n, nbins, K, true, false), [&](hipStream_t st, const uint32_t *, char *work) {
        return cl_seed_launch(st, n, nbins, hist_d, K, (uint32_t)seed, (uint32_t)(seed >> 32), nonce, centroids_d, cl_work(work, n, nbins, K, true, false));
    });
}

int pk_hist_cluster_assign_d(int device, size_t n, int nbins, const uint16_t *hist_d, int K, const uint16_t *centroids_d, uint16_t *label_d,
                             uint32_t *dist_d, void *stream) {
    const char *call = "pk_hist_cluster_assign_d";
    EQ_REFUSE(g_fail, call, cl_check(n, nbins, K, hist_d && centroids_d && label_d));
    return eq_call_d(call, device, stream, n, EQ_TAB_NONE, cl_work_bytes(n, nbins, K, false, false), [&](hipStream_t st, const uint32_t *, char *work) {
        return cl_assign_launch(st, n, nbins, hist_d, K, centroids_d, label_d, dist_d, cl_work(work, n, nbins, K, false, false));
    });
}

int pk_hist_cluster_d(int device, size_t n, int nbins, const uint16_t *hist_d, int K, uint16_t *centroids_d, int iters, uint16_t *label_d,
                      uint32_t *dist_d, uint64_t *inertia_d, uint32_t *changed_d, void *stream) {
    const char *call = "pk_hist_cluster_d";
    EQ_REFUSE(g_fail, call, cl_check(n, nbins, K, hist_d && centroids_d && label_d));
    EQ_REFUSE(g_fail, call, cl_bad_k_rows(n, K));
    EQ_REFUSE(g_fail, call, cl_bad_iters(iters));
    return eq_call_d(call, device, stream, n, EQ_TAB_NONE, cl_work_bytes(n, nbins, K, false, true), [&](hipStream_t st, const uint32_t *, char *work) {
        return cl_cluster_launch(st, n, nbins, hist_d, K, centroids_d, iters, label_d, dist_d, inertia_d, changed_d, cl_work(work, n, nbins, K, false, true));
    });
}

int pk_hist_cluster_seed(int device, size_t n, int nbins, const uint16_t *hist, int K, uint64_t seed, uint32_t nonce, uint16_t *centroids) {
    const char *call = "pk_hist_cluster_seed";
    EQ_REFUSE(g_fail, call, cl_check(n, nbins, K, hist && centroids));
    EQ_REFUSE(g_fail, call, cl_bad_k_rows(n, K));
    EQ_REFUSE(g_fail, call, cl_bad_rows(n, nbins, hist, K));
    Stage g;
    const int hi = g.in(hist, n * (size_t)nbins * 2), ce = g.out(centroids, (size_t)K * nbins * 2);
    return eq_call_host(call, device, n, EQ_TAB_NONE, g, cl_work_bytes(n, nbins, K, true, false), [&](hipStream_t st, const uint32_t *, char *work) {
        return cl_seed_launch(st, n, nbins, g.at<uint16_t>(hi), K, (uint32_t)seed, (uint32_t)(seed >> 32), nonce, g.at<uint16_t>(ce), cl_work(work, n, nbins, K, true, false));
    });
}

int pk_hist_cluster_assign(int device, size_t n, int nbins, const uint16_t *hist, int K, const uint16_t *centroids, uint16_t *label, uint32_t *dist) {
    const char *call = "pk_hist_cluster_assign";
    EQ_REFUSE(g_fail, call, cl_check(n, nbins, K, hist && centroids && label));
    Stage g;
    const int hi = g.in(hist, n * (size_t)nbins * 2), ce = g.in(centroids, (size_t)K * nbins * 2), la = g.out(label, n * 2), di = g.out(dist, n * 4);
    return eq_call_host(call, device, n, EQ_TAB_NONE, g, cl_work_bytes(n, nbins, K, false, false), [&](hipStream_t st, const uint32_t *, char *work) {
        return cl_assign_launch(st, n, nbins, g.at<uint16_t>(hi), K, g.at<uint16_t>(ce), g.at<uint16_t>(la), g.at<uint32_t>(di), cl_work(work, n, nbins, K, false, false));
    });
}

int pk_hist_cluster(int device, size_t n, int nbins, const uint16_t *hist, int K, uint16_t *centroids, int iters, uint16_t *label, uint32_t *dist,
                    uint64_t *inertia, uint32_t *changed) {
    const char *call = "pk_hist_cluster";
    EQ_REFUSE(g_fail, call, cl_check(n, nbins, K, hist && centroids && label));
    EQ_REFUSE(g_fail, call, cl_bad_k_rows(n, K));
    EQ_REFUSE(g_fail, call, cl_bad_iters(iters));
    EQ_REFUSE(g_fail, call, cl_bad_rows(n, nbins, hist, K));
    Stage g;
    const int hi = g.in(hist, n * (size_t)nbins * 2), ce = g.add((size_t)K * nbins * 2, centroids, centroids), la = g.out(label, n * 2), di = g.out(dist, n * 4);
    const int in = g.out(inertia, (size_t)(iters + 1) * 8), ch = g.out(changed, (size_t)iters * 4);
    return eq_call_host(call, device, n, EQ_TAB_NONE, g, cl_work_bytes(n, nbins, K, false, true), [&](hipStream_t st, const uint32_t *, char *work) {
        return cl_cluster_launch(st, n, nbins, g.at<uint16_t>(hi), K, g.at<uint16_t>(ce), iters, g.at<uint16_t>(la), g.at<uint32_t>(di), g.at<uint64_t>(in),
                                 g.at<uint32_t>(ch), cl_work(work, n, nbins, K, false, true));
    });
}

// ---- pre-flop matchups (pokerl_hip.h "Pre-flop matchups"; kernels: pk_preflop.hip).  The count pass's work space: the keys of one chunk of
// boards (knob PK_PFM_CHUNK, boards).  The readers' work space: one holding index per spot.
static uint32_t pfm_chunk() { return (uint32_t)env_int("PK_PFM_CHUNK", 1, PFM_CHUNK_MAX, PFM_CHUNK_DEFAULT); }
// The matchup table, one per device, built on first use on `stream` (the device is current): the partial count over all boards.  The
// build's key work space is allocated for the build and freed after it: only the table stays.
static std::mutex g_pfm_mu;
static DevBuf g_pfm_tab[PK_MAX_DEVICES];
static const uint32_t *pfm_table(int device, hipStream_t stream) {
    if (device < 0 || device >= PK_MAX_DEVICES) return nullptr;
    std::lock_guard<std::mutex> lock(g_pfm_mu);
    DevBuf &t = g_pfm_tab[device];
    if (!t.alive()) {   // (not yet there, or the device was reset: build it)
        t = DevBuf{};
        const uint32_t *tab = eval7_table(device, stream);
        if (!tab) return nullptr;
        const uint32_t chunk = pfm_chunk();
        DevBuf keys;                                 // (the build's own: 92 MB at the default chunk, freed once the table stands)
        uint32_t *kp = (uint32_t *)keys.reserve(pfm_keys_bytes(chunk), pfm_keys_bytes(chunk), stream);
        uint32_t *p = kp ? (uint32_t *)t.reserve(2 * PFM_CELLS * 4, 2 * PFM_CELLS * 4, stream, true) : nullptr;
        const bool ok = p && pfm_count_launch(stream, tab, 0, PFM_BOARDS, 0, chunk, kp, p, p + PFM_CELLS) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
        keys.drop();
        if (!ok) {
            (void)hipGetLastError();
            t.drop();
            return nullptr;
        }
    }
    return (const uint32_t *)t.p;
}

static const char *pfm_count_check(uint32_t first, uint32_t n) {
    return (uint64_t)first + n > (uint64_t)PFM_BOARDS ? ": first + n above PK_PREFLOP_ALL_BOARDS (2 598 960)" : nullptr;
}

int pk_preflop_count_d(int device, uint32_t first, uint32_t n, int accumulate, uint32_t *win_d, uint32_t *tie_d, void *stream) {
    const char *call = "pk_preflop_count_d";
    EQ_REFUSE(g_fail, call, pfm_count_check(first, n));
    const uint32_t chunk = pfm_chunk();
    return eq_call_d(call, device, stream, n, EQ_TAB_EVAL, pfm_keys_bytes(chunk), [&](hipStream_t st, const uint32_t *tab, char *work) {
        return pfm_count_launch(st, tab, first, n, accumulate, chunk, (uint32_t *)work, win_d, tie_d);
    });
}

int pk_preflop_count(int device, uint32_t first, uint32_t n, int accumulate, uint32_t *win, uint32_t *tie) {
    const char *call = "pk_preflop_count";
    EQ_REFUSE(g_fail, call, pfm_count_check(first, n));
    const uint32_t chunk = pfm_chunk();
    Stage g;   // (an accumulating call uploads what the arrays hold)
    const int wi = win ? g.add(PFM_CELLS * 4, accumulate ? win : nullptr, win) : -1, ti = tie ? g.add(PFM_CELLS * 4, accumulate ? tie : nullptr, tie) : -1;
    return eq_call_host(call, device, n, EQ_TAB_EVAL, g, pfm_keys_bytes(chunk), [&](hipStream_t st, const uint32_t *tab, char *work) {
        return pfm_count_launch(st, tab, first, n, accumulate, chunk, (uint32_t *)work, g.at<uint32_t>(wi), g.at<uint32_t>(ti));
    });
}

int pk_preflop_matchups_d(int device, uint32_t *win_d, uint32_t *tie_d, void *stream) {
    const char *call = "pk_preflop_matchups_d";
    return eq_call_d(call, device, stream, (win_d || tie_d) ? 1 : 0, EQ_TAB_PREFLOP, 0, [&](hipStream_t st, const uint32_t *M, char *) {
        hipError_t e = hipSuccess;
        if (win_d) e = hipMemcpyAsync(win_d, M, PFM_CELLS * 4, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && tie_d) e = hipMemcpyAsync(tie_d, M + PFM_CELLS, PFM_CELLS * 4, hipMemcpyDeviceToDevice, st);
        return e;
    });
}

int pk_preflop_matchups(int device, uint32_t *win, uint32_t *tie) {
    const char *call = "pk_preflop_matchups";
    Stage g;
    const int wi = g.out(win, PFM_CELLS * 4), ti = g.out(tie, PFM_CELLS * 4);
    return eq_call_host(call, device, (win || tie) ? 1 : 0, EQ_TAB_PREFLOP, g, 0, [&](hipStream_t st, const uint32_t *M, char *) {
        hipError_t e = hipSuccess;
        if (win) e = hipMemcpyAsync(g.at<uint32_t>(wi), M, PFM_CELLS * 4, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && tie) e = hipMemcpyAsync(g.at<uint32_t>(ti), M + PFM_CELLS, PFM_CELLS * 4, hipMemcpyDeviceToDevice, st);
        return e;
    });
}

// boards / status alone are the preparation kernel's: such a call neither reads nor builds the table
static int pfm_hero_needs(const void *agg, const void *win, const void *tie) { return agg || win || tie ? EQ_TAB_PREFLOP : EQ_TAB_NONE; }
static const char *pfm_hero_check(size_t m, bool inputs) {
    if (const char *why = eq_bad_m(m)) return why;
    return eq_null(m, inputs);
}

int pk_equity_preflop_d(int device, size_t m, const uint8_t *hero_d, const uint16_t *weights_d, int weights_per_spot, uint64_t *agg_d, uint32_t *win_d,
                        uint32_t *tie_d, uint32_t *boards_d, uint8_t *status_d, void *stream) {
    const char *call = "pk_equity_preflop_d";
    EQ_REFUSE(g_fail, call, pfm_hero_check(m, hero_d != nullptr));
    return eq_call_d(call, device, stream, m, pfm_hero_needs(agg_d, win_d, tie_d), pfm_desc_bytes(m), [&](hipStream_t st, const uint32_t *M, char *work) {
        return pfm_hero_launch(st, M, hero_d, nullptr, 0, PK_OBSERVER_NONE, PfmWeights{weights_d, weights_per_spot != 0}, m,
                               PfmOut{agg_d, win_d, tie_d, boards_d, status_d}, (uint32_t *)work);
    });
}

int pk_equity_preflop(int device, size_t m, const uint8_t *hero, const uint16_t *weights, int weights_per_spot, uint64_t *agg, uint32_t *win,
                      uint32_t *tie, uint32_t *boards, uint8_t *status) {
    const char *call = "pk_equity_preflop";
    EQ_REFUSE(g_fail, call, pfm_hero_check(m, hero != nullptr));
    Stage g;
    const int he = g.in(hero, m * 2), we = g.in(weights, eqr_weight_bytes(m, weights_per_spot));
    const EqrStagedOut out(g, m, agg, win, tie, boards, status);
    return eq_call_host(call, device, m, pfm_hero_needs(agg, win, tie), g, pfm_desc_bytes(m), [&](hipStream_t st, const uint32_t *M, char *work) {
        const EqrOut o = out.at(g);
        return pfm_hero_launch(st, M, g.at<uint8_t>(he), nullptr, 0, PK_OBSERVER_NONE, PfmWeights{g.at<uint16_t>(we), weights_per_spot != 0}, m,
                               PfmOut{o.agg, o.win, o.tie, o.boards, o.status}, (uint32_t *)work);
    });
}

int pk_table_equity_preflop_d(pk_handle *h, const int32_t *tables_d, size_t m, int observer, const uint16_t *weights_d, int weights_per_spot,
                              uint64_t *agg_d, uint32_t *win_d, uint32_t *tie_d, uint32_t *boards_d, uint8_t *status_d) {
    const char *call = "pk_table_equity_preflop_d";
    if (!h) return g_fail(PK_E_INVALID_ARG, "pk_table_equity_preflop_d: NULL handle");
    EQ_REFUSE(h->fail, call, eqr_table_check(h, m, observer));
    return eq_table_call_d(h, call, tables_d, m, pfm_hero_needs(agg_d, win_d, tie_d), pfm_desc_bytes(m), [&](const uint32_t *M, const EqTables &t, char *work) {
        return pfm_hero_launch(h->stream, M, nullptr, &t, h->N, observer, PfmWeights{weights_d, weights_per_spot != 0}, m,
                               PfmOut{agg_d, win_d, tie_d, boards_d, status_d}, (uint32_t *)work);
    });
}

int pk_table_equity_preflop(pk_handle *h, const int32_t *tables, size_t m, int observer, const uint16_t *weights, int weights_per_spot, uint64_t *agg,
                            uint32_t *win, uint32_t *tie, uint32_t *boards, uint8_t *status) {
    const char *call = "pk_table_equity_preflop";
    if (!h) return g_fail(PK_E_INVALID_ARG, "pk_table_equity_preflop: NULL handle");
    EQ_REFUSE(h->fail, call, eqr_table_check(h, m, observer));
    Stage g;
    const int we = g.in(weights, eqr_weight_bytes(m, weights_per_spot));
    const EqrStagedOut out(g, m, agg, win, tie, boards, status);
    return eq_table_call(h, call, tables, m, pfm_hero_needs(agg, win, tie), g, pfm_desc_bytes(m), [&](const uint32_t *M, const EqTables &t, char *work) {
        const EqrOut o = out.at(g);
        return pfm_hero_launch(h->stream, M, nullptr, &t, h->N, observer, PfmWeights{g.at<uint16_t>(we), weights_per_spot != 0}, m,
                               PfmOut{o.agg, o.win, o.tie, o.boards, o.status}, (uint32_t *)work);
    });
}

int pk_equity_rvr_preflop_d(int device, size_t m, const uint16_t *weights_d, uint64_t *win_d, uint64_t *tie_d, uint64_t *tot_d, void *stream) {
    const char *call = "pk_equity_rvr_preflop_d";
    EQ_REFUSE(g_fail, call, eq_bad_m(m));
    return eq_call_d(call, device, stream, m, EQ_TAB_PREFLOP, 0, [&](hipStream_t st, const uint32_t *M, char *) {
        return pfm_rvr_launch(st, M, weights_d, m, win_d, tie_d, tot_d);
    });
}

int pk_equity_rvr_preflop(int device, size_t m, const uint16_t *weights, uint64_t *win, uint64_t *tie, uint64_t *tot) {
    const char *call = "pk_equity_rvr_preflop";
    EQ_REFUSE(g_fail, call, eq_bad_m(m));
    Stage g;
    const int we = g.in(weights, m * PFM_HOLDINGS * 2);
    const int wi = g.out(win, m * PFM_HOLDINGS * 8), ti = g.out(tie, m * PFM_HOLDINGS * 8), to = g.out(tot, m * PFM_HOLDINGS * 8);
    return eq_call_host(call, device, m, EQ_TAB_PREFLOP, g, 0, [&](hipStream_t st, const uint32_t *M, char *) {
        return pfm_rvr_launch(st, M, g.at<uint16_t>(we), m, g.at<uint64_t>(wi), g.at<uint64_t>(ti), g.at<uint64_t>(to));
    });
}

// ---- the river solver (pokerl_hip.h "River solver"; kernels: pk_river_solver.hip).  The tree is checked and packed on the host and travels
// with the launch; the work space is the descriptors plus a slice per resident workgroup.  There is no table form.
static_assert(RS_HOLDINGS == PK_EQ_HOLDINGS, "pk_river_solver.hpp and the ABI header agree");
// The tree check: the refusal's text, or NULL with `t` filled (nact and row derived)
// (resolve: the re-solving call's check, which also takes one terminal of kind RS_GIVEN -- pokerl_hip.h "Re-solving"; *given: the tree has one)
static const char *rs_check_tree(uint32_t n, const uint8_t *kind, const uint8_t *child, const uint32_t *put, uint32_t pot, RsTree &t, bool resolve = false,
                                 bool *given = nullptr) {
    if (n < 1u || n > (uint32_t)RS_MAX_NODES) return ": n outside 1 .. 64";
    t = RsTree{};
    t.n = n; t.pot = pot;
    uint32_t parents[RS_MAX_NODES] = {0}, rows = 0, givens = 0;
    for (uint32_t v = 0; v < n; ++v) {
        if (resolve && kind[v] == RS_GIVEN) {
            if (++givens > 1u) return ": more than one given node";
        } else if (kind[v] > RS_SHOWDOWN) return resolve ? ": a node kind outside 0 .. 4 and not 6" : ": a node kind outside 0 .. 4";
        if (v == 0 && kind[v] > RS_P1) return ": the root is not a decision node";
        t.kind[v] = kind[v];
        t.put[v][0] = put[v * 2]; t.put[v][1] = put[v * 2 + 1];
        const uint32_t top = put[v * 2] > put[v * 2 + 1] ? put[v * 2] : put[v * 2 + 1];
        if (pot > RS_MAX_CHIPS || top > RS_MAX_CHIPS || pot + top > RS_MAX_CHIPS) return ": pot + max put > 8191";
        if (kind[v] == RS_SHOWDOWN && put[v * 2] != put[v * 2 + 1]) return ": a showdown has put[0] != put[1]";
        uint32_t nact = 0;
        bool ended = false;
        for (int a = 0; a < 4; ++a) {
            const uint32_t c = child[v * 4 + a];
            t.child[v][a] = (uint8_t)c;
            if (c == 0xFFu) { ended = true; continue; }
            if (kind[v] > RS_P1) return ": a terminal has a child";
            if (ended) return ": a node's children are not packed first";
            if (c <= v || c >= n) return ": a child index is <= its parent or >= n";
            ++parents[c];
            ++nact;
        }
        if (kind[v] <= RS_P1 && nact == 0u) return ": a decision node has no child";
        t.nact[v] = (uint8_t)nact;
        if (kind[v] <= RS_P1) t.row[v] = (uint8_t)rows++;
    }
    for (uint32_t v = 1; v < n; ++v)
        if (parents[v] != 1u) return ": a non-root node does not have exactly one parent";
    if (given) *given = givens != 0u;
    return nullptr;
}
static const char *rs_check(size_t m, bool pointers, uint32_t iters, uint32_t n, const uint8_t *kind, const uint8_t *child, const uint32_t *put,
                            uint32_t pot, RsTree &t) {
    if (const char *why = eq_bad_m(m)) return why;
    if ((m && !pointers) || !kind || !child || !put) return ": NULL where a pointer is required (board, ranges, kind, child, put, status)";
    if (iters < 1u || iters > (uint32_t)RS_MAX_ITERS) return ": iters outside 1 .. 4096";
    return rs_check_tree(n, kind, child, put, pot, t);
}

int pk_solve_river_d(int device, size_t m, const uint8_t *board_d, const uint64_t *dead_d, const uint16_t *ranges_d, uint32_t n, const uint8_t *kind,
                     const uint8_t *child, const uint32_t *put, uint32_t pot, uint32_t iters, uint16_t *strategy_d, int64_t *value_d, int64_t *br_d,
                     uint8_t *status_d, void *stream) {
    const char *call = "pk_solve_river_d";
    RsTree t;
    EQ_REFUSE(g_fail, call, rs_check(m, board_d && ranges_d && status_d, iters, n, kind, child, put, pot, t));
    const bool solve = strategy_d || value_d || br_d;
    return eq_call_d(call, device, stream, m, EQ_TAB_EVAL, rs_work_bytes(m, n, solve), [&](hipStream_t st, const uint32_t *tab, char *work) {
        return rs_launch(st, tab, RsSpots{board_d, dead_d, ranges_d}, t, iters, m, RsOut{strategy_d, value_d, br_d, status_d}, work);
    });
}

int pk_solve_river(int device, size_t m, const uint8_t *board, const uint64_t *dead, const uint16_t *ranges, uint32_t n, const uint8_t *kind,
                   const uint8_t *child, const uint32_t *put, uint32_t pot, uint32_t iters, uint16_t *strategy, int64_t *value, int64_t *br,
                   uint8_t *status) {
    const char *call = "pk_solve_river";
    RsTree t;
    EQ_REFUSE(g_fail, call, rs_check(m, board && ranges && status, iters, n, kind, child, put, pot, t));
    size_t D = 0;
    for (uint32_t v = 0; v < n; ++v) D += t.kind[v] <= RS_P1;
    const bool solve = strategy || value || br;
    Stage g;
    const int bo = g.in(board, m * 5), de = g.in(dead, m * 8), ra = g.in(ranges, m * 2 * RS_HOLDINGS * 2);
    const int sg = g.out(strategy, m * D * 4 * RS_HOLDINGS * 2), va = g.out(value, m * 2 * RS_HOLDINGS * 8), be = g.out(br, m * 2 * RS_HOLDINGS * 8);
    const int su = g.out(status, m);
    return eq_call_host(call, device, m, EQ_TAB_EVAL, g, rs_work_bytes(m, n, solve), [&](hipStream_t st, const uint32_t *tab, char *work) {
        return rs_launch(st, tab, RsSpots{g.at<uint8_t>(bo), g.at<uint64_t>(de), g.at<uint16_t>(ra)}, t, iters, m,
                         RsOut{g.at<uint16_t>(sg), g.at<int64_t>(va), g.at<int64_t>(be), g.at<uint8_t>(su)}, work);
    });
}

// ---- the turn solver (pokerl_hip.h "Turn solver"; kernels: pk_turn_solver.hip).  As the river solver: the tree is checked and packed on
// the host and travels with the launch (TsTree fits the kernel-argument space beside the other arguments; the static_assert of
// pk_turn_solver.hpp holds it there); the work space is the descriptors plus a slice per resident workgroup.
// The tree check: the refusal's text, or NULL with `t` filled (nact, row, river and idx derived)
static const char *ts_check_tree(uint32_t n, const uint8_t *kind, const uint8_t *child, const uint32_t *put, uint32_t pot, TsTree &t) {
    if (n < 1u || n > (uint32_t)TS_MAX_NODES) return ": n outside 1 .. 128";
    t = TsTree{};
    t.n = n; t.pot = pot;
    uint32_t parents[TS_MAX_NODES] = {0}, rows[2] = {0, 0};
    for (uint32_t v = 0; v < n; ++v) {
        if (kind[v] > TS_CHANCE) return ": a node kind outside 0 .. 5";
        if (v == 0 && kind[v] > RS_P1) return ": the root is not a decision node";
        t.kind[v] = kind[v];
        t.put[v][0] = put[v * 2]; t.put[v][1] = put[v * 2 + 1];
        const uint32_t top = put[v * 2] > put[v * 2 + 1] ? put[v * 2] : put[v * 2 + 1];
        if (pot > RS_MAX_CHIPS || top > RS_MAX_CHIPS || pot + top > RS_MAX_CHIPS) return ": pot + max put > 8191";
        if (kind[v] == RS_SHOWDOWN && put[v * 2] != put[v * 2 + 1]) return ": a showdown has put[0] != put[1]";
        if (kind[v] == TS_CHANCE && put[v * 2] != put[v * 2 + 1]) return ": a chance node has put[0] != put[1]";
        const bool terminal = kind[v] > RS_P1 && kind[v] != TS_CHANCE;
        uint32_t nact = 0;
        bool ended = false;
        for (int a = 0; a < 4; ++a) {
            const uint32_t c = child[v * 4 + a];
            t.child[v][a] = (uint8_t)c;
            if (c == 0xFFu) { ended = true; continue; }
            if (terminal) return ": a terminal has a child";
            if (ended) return ": a node's children are not packed first";
            if (c <= v || c >= n) return ": a child index is <= its parent or >= n";
            ++parents[c];
            ++nact;
        }
        if (kind[v] <= RS_P1 && nact == 0u) return ": a decision node has no child";
        if (kind[v] == TS_CHANCE && nact != 1u) return ": a chance node does not have exactly one child";
        t.nact[v] = (uint8_t)nact;
    }
    for (uint32_t v = 1; v < n; ++v)
        if (parents[v] != 1u) return ": a non-root node does not have exactly one parent";
    // the levels (every parent comes before its children), then what is counted per level
    for (uint32_t v = 0; v < n; ++v) {
        if (kind[v] == TS_CHANCE && t.river[v]) return ": a chance node below a chance node";
        if (kind[v] == RS_SHOWDOWN && !t.river[v]) return ": a turn-level showdown";
        for (uint32_t a = 0; a < t.nact[v]; ++a) t.river[t.child[v][a]] = (uint8_t)(t.river[v] || kind[v] == TS_CHANCE);
        uint32_t &count = t.river[v] ? t.nr : t.nt;
        t.idx[v] = (uint8_t)count++;
        if (kind[v] <= RS_P1) t.row[v] = (uint8_t)rows[t.river[v]]++;
    }
    return nullptr;
}
static const char *ts_check(size_t m, bool pointers, uint32_t iters, uint32_t n, const uint8_t *kind, const uint8_t *child, const uint32_t *put,
                            uint32_t pot, TsTree &t) {
    if (const char *why = eq_bad_m(m)) return why;
    if ((m && !pointers) || !kind || !child || !put) return ": NULL where a pointer is required (board, ranges, kind, child, put, status)";
    if (iters < 1u || iters > (uint32_t)RS_MAX_ITERS) return ": iters outside 1 .. 4096";
    return ts_check_tree(n, kind, child, put, pot, t);
}

unsigned pk_turn_grid(size_t m, uint32_t nt, uint32_t nr) { return ts_grid(m, nt, nr); }

int pk_solve_turn_d(int device, size_t m, const uint8_t *board_d, const uint64_t *dead_d, const uint16_t *ranges_d, uint32_t n, const uint8_t *kind,
                    const uint8_t *child, const uint32_t *put, uint32_t pot, uint32_t iters, uint16_t *strategy_d, uint16_t *river_strategy_d,
                    int64_t *value_d, int64_t *br_d, uint8_t *status_d, void *stream) {
    const char *call = "pk_solve_turn_d";
    TsTree t;
    EQ_REFUSE(g_fail, call, ts_check(m, board_d && ranges_d && status_d, iters, n, kind, child, put, pot, t));
    const bool solve = strategy_d || river_strategy_d || value_d || br_d;
    return eq_call_d(call, device, stream, m, EQ_TAB_EVAL, ts_work_bytes(m, t.nt, t.nr, solve), [&](hipStream_t st, const uint32_t *tab, char *work) {
        return ts_launch(st, tab, TsSpots{board_d, dead_d, ranges_d}, t, iters, m, TsOut{strategy_d, river_strategy_d, value_d, br_d, status_d}, work);
    });
}

int pk_solve_turn(int device, size_t m, const uint8_t *board, const uint64_t *dead, const uint16_t *ranges, uint32_t n, const uint8_t *kind,
                  const uint8_t *child, const uint32_t *put, uint32_t pot, uint32_t iters, uint16_t *strategy, uint16_t *river_strategy,
                  int64_t *value, int64_t *br, uint8_t *status) {
    const char *call = "pk_solve_turn";
    TsTree t;
    EQ_REFUSE(g_fail, call, ts_check(m, board && ranges && status, iters, n, kind, child, put, pot, t));
    size_t Dt = 0, Dr = 0;
    for (uint32_t v = 0; v < n; ++v) (t.river[v] ? Dr : Dt) += t.kind[v] <= RS_P1;
    const bool solve = strategy || river_strategy || value || br;
    Stage g;
    const int bo = g.in(board, m * 4), de = g.in(dead, m * 8), ra = g.in(ranges, m * 2 * RS_HOLDINGS * 2);
    const int sg = g.out(strategy, m * Dt * 4 * RS_HOLDINGS * 2), rg = g.out(river_strategy, m * Dr * 52 * 4 * RS_HOLDINGS * 2);
    const int va = g.out(value, m * 2 * RS_HOLDINGS * 8), be = g.out(br, m * 2 * RS_HOLDINGS * 8), su = g.out(status, m);
    return eq_call_host(call, device, m, EQ_TAB_EVAL, g, ts_work_bytes(m, t.nt, t.nr, solve), [&](hipStream_t st, const uint32_t *tab, char *work) {
        return ts_launch(st, tab, TsSpots{g.at<uint8_t>(bo), g.at<uint64_t>(de), g.at<uint16_t>(ra)}, t, iters, m,
                         TsOut{g.at<uint16_t>(sg), g.at<uint16_t>(rg), g.at<int64_t>(va), g.at<int64_t>(be), g.at<uint8_t>(su)}, work);
    });
}

// ---- the river and turn solvers with a tree per spot (pokerl_hip.h "River and turn solvers: a tree per spot").
// Every tree is checked and packed on the host with the one-tree calls' checks; the packed trees go to the device with the call -- in the
// host forms as a piece of the staging, in the device forms behind the work space on the caller's stream (the source is this call's own
// pageable vector: the runtime has finished with it when hipMemcpyAsync returns, so it may go when the call does).
static_assert(RS_MAX_TREES == 65536u, "the header's text names the limit");
struct RsPacked { std::vector<RsTree> trees; uint32_t nmax = 0, Dmax = 0; bool given = false; std::string why; };
struct TsPacked { std::vector<TsTree> trees; uint32_t ntmax = 0, nrmax = 0, Dtmax = 0, Drmax = 0; std::string why; };
static const char *trees_check(size_t m, bool pointers, uint32_t iters, uint32_t ntrees, bool tree_pointers) {
    if (const char *why = eq_bad_m(m)) return why;
    if ((m && !pointers) || !tree_pointers) return ": NULL where a pointer is required (board, ranges, n, kind, child, put, pot, tree_of, status)";
    if (iters < 1u || iters > (uint32_t)RS_MAX_ITERS) return ": iters outside 1 .. 4096";
    if (ntrees < 1u || ntrees > RS_MAX_TREES) return ": ntrees outside 1 .. 65536";
    return nullptr;
}
static const char *trees_refusal(std::string &text, uint32_t k, const char *why) {
    text = ": tree " + std::to_string(k) + why;
    return text.c_str();
}
static const char *rs_pack_trees(size_t m, bool pointers, uint32_t iters, uint32_t ntrees, const uint32_t *n, const uint8_t *kind, const uint8_t *child,
                                 const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of, RsPacked &p, bool resolve = false) {
    if (const char *why = trees_check(m, pointers, iters, ntrees, n && kind && child && put && pot && tree_of)) return why;
    p.trees.resize(ntrees);
    for (uint32_t k = 0; k < ntrees; ++k) {
        const size_t row = (size_t)k * RS_MAX_NODES;
        bool given = false;
        if (const char *why = rs_check_tree(n[k], kind + row, child + row * 4, put + row * 2, pot[k], p.trees[k], resolve, &given)) return trees_refusal(p.why, k, why);
        p.given = p.given || given;
        uint32_t D = 0;
        for (uint32_t v = 0; v < n[k]; ++v) D += p.trees[k].kind[v] <= RS_P1;
        p.nmax = n[k] > p.nmax ? n[k] : p.nmax;
        p.Dmax = D > p.Dmax ? D : p.Dmax;
    }
    return nullptr;
}
static const char *ts_pack_trees(size_t m, bool pointers, uint32_t iters, uint32_t ntrees, const uint32_t *n, const uint8_t *kind, const uint8_t *child,
                                 const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of, TsPacked &p) {
    if (const char *why = trees_check(m, pointers, iters, ntrees, n && kind && child && put && pot && tree_of)) return why;
    p.trees.resize(ntrees);
    for (uint32_t k = 0; k < ntrees; ++k) {
        const size_t row = (size_t)k * TS_MAX_NODES;
        TsTree &t = p.trees[k];
        if (const char *why = ts_check_tree(n[k], kind + row, child + row * 4, put + row * 2, pot[k], t)) return trees_refusal(p.why, k, why);
        uint32_t D[2] = {0, 0};
        for (uint32_t v = 0; v < n[k]; ++v) D[t.river[v]] += t.kind[v] <= RS_P1;
        p.ntmax = t.nt > p.ntmax ? t.nt : p.ntmax;
        p.nrmax = t.nr > p.nrmax ? t.nr : p.nrmax;
        p.Dtmax = D[0] > p.Dtmax ? D[0] : p.Dtmax;
        p.Drmax = D[1] > p.Drmax ? D[1] : p.Drmax;
    }
    return nullptr;
}

int pk_rs_trees_rows(uint32_t ntrees, const uint32_t *n, const uint8_t *kind, uint32_t *Dmax) {
    const char *call = "pk_rs_trees_rows";
    if (ntrees < 1u || ntrees > RS_MAX_TREES || !n || !kind || !Dmax) return eq_fail(PK_E_INVALID_ARG, call, ": ntrees outside 1 .. 65536, or a NULL pointer");
    uint32_t best = 0;
    for (uint32_t k = 0; k < ntrees; ++k) {
        if (n[k] < 1u || n[k] > (uint32_t)RS_MAX_NODES) return eq_fail(PK_E_INVALID_ARG, call, (": tree " + std::to_string(k) + ": n outside 1 .. 64").c_str());
        uint32_t D = 0;
        for (uint32_t v = 0; v < n[k]; ++v) D += kind[(size_t)k * RS_MAX_NODES + v] <= RS_P1;
        best = D > best ? D : best;
    }
    *Dmax = best;
    return PK_OK;
}

int pk_ts_trees_rows(uint32_t ntrees, const uint32_t *n, const uint8_t *kind, const uint8_t *child, uint32_t *Dtmax, uint32_t *Drmax) {
    const char *call = "pk_ts_trees_rows";
    if (ntrees < 1u || ntrees > RS_MAX_TREES || !n || !kind || !child || !Dtmax || !Drmax)
        return eq_fail(PK_E_INVALID_ARG, call, ": ntrees outside 1 .. 65536, or a NULL pointer");
    uint32_t best[2] = {0, 0};
    for (uint32_t k = 0; k < ntrees; ++k) {
        if (n[k] < 1u || n[k] > (uint32_t)TS_MAX_NODES) return eq_fail(PK_E_INVALID_ARG, call, (": tree " + std::to_string(k) + ": n outside 1 .. 128").c_str());
        const uint8_t *kd = kind + (size_t)k * TS_MAX_NODES, *ch = child + (size_t)k * TS_MAX_NODES * 4;
        uint8_t river[TS_MAX_NODES] = {0};
        uint32_t D[2] = {0, 0};
        for (uint32_t v = 0; v < n[k]; ++v) {                 // (every parent comes before its children: the level of v is known here)
            for (int a = 0; a < 4; ++a) {
                const uint32_t c = ch[v * 4 + a];
                if (c == 0xFFu) continue;
                if (c <= v || c >= n[k]) return eq_fail(PK_E_INVALID_ARG, call, (": tree " + std::to_string(k) + ": a child index is <= its parent or >= n").c_str());
                river[c] = (uint8_t)(river[v] || kd[v] == TS_CHANCE);
            }
            D[river[v]] += kd[v] <= RS_P1;
        }
        best[0] = D[0] > best[0] ? D[0] : best[0];
        best[1] = D[1] > best[1] ? D[1] : best[1];
    }
    *Dtmax = best[0]; *Drmax = best[1];
    return PK_OK;
}

int pk_solve_river_trees_d(int device, size_t m, const uint8_t *board_d, const uint64_t *dead_d, const uint16_t *ranges_d, uint32_t ntrees, const uint32_t *n,
                           const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of_d, uint32_t iters,
                           uint16_t *strategy_d, int64_t *value_d, int64_t *br_d, uint8_t *status_d, void *stream) {
    const char *call = "pk_solve_river_trees_d";
    RsPacked p;
    EQ_REFUSE(g_fail, call, rs_pack_trees(m, board_d && ranges_d && status_d, iters, ntrees, n, kind, child, put, pot, tree_of_d, p));
    const bool solve = strategy_d || value_d || br_d;
    const size_t ws = rs_work_bytes(m, p.nmax, solve);
    return eq_call_d(call, device, stream, m, EQ_TAB_EVAL, ws + (solve ? rs_trees_bytes(ntrees) : 0), [&](hipStream_t st, const uint32_t *tab, char *work) {
        RsTree *trees_d = (RsTree *)(work + ws);
        if (solve)
            if (const hipError_t e = hipMemcpyAsync(trees_d, p.trees.data(), (size_t)ntrees * sizeof(RsTree), hipMemcpyHostToDevice, st)) return e;
        return rs_launch_trees(st, tab, RsSpots{board_d, dead_d, ranges_d}, RsTrees{trees_d, tree_of_d, p.nmax, p.Dmax}, ntrees, iters, m,
                               RsOut{strategy_d, value_d, br_d, status_d}, work);
    });
}

int pk_solve_river_trees(int device, size_t m, const uint8_t *board, const uint64_t *dead, const uint16_t *ranges, uint32_t ntrees, const uint32_t *n,
                         const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of, uint32_t iters,
                         uint16_t *strategy, int64_t *value, int64_t *br, uint8_t *status) {
    const char *call = "pk_solve_river_trees";
    RsPacked p;
    EQ_REFUSE(g_fail, call, rs_pack_trees(m, board && ranges && status, iters, ntrees, n, kind, child, put, pot, tree_of, p));
    const bool solve = strategy || value || br;
    Stage g;
    const int bo = g.in(board, m * 5), de = g.in(dead, m * 8), ra = g.in(ranges, m * 2 * RS_HOLDINGS * 2), to = g.in(tree_of, m * 4);
    const int tr = g.in(solve ? p.trees.data() : nullptr, (size_t)ntrees * sizeof(RsTree));
    const int sg = g.out(strategy, m * p.Dmax * 4 * RS_HOLDINGS * 2), va = g.out(value, m * 2 * RS_HOLDINGS * 8), be = g.out(br, m * 2 * RS_HOLDINGS * 8);
    const int su = g.out(status, m);
    return eq_call_host(call, device, m, EQ_TAB_EVAL, g, rs_work_bytes(m, p.nmax, solve), [&](hipStream_t st, const uint32_t *tab, char *work) {
        return rs_launch_trees(st, tab, RsSpots{g.at<uint8_t>(bo), g.at<uint64_t>(de), g.at<uint16_t>(ra)},
                               RsTrees{g.at<RsTree>(tr), g.at<uint32_t>(to), p.nmax, p.Dmax}, ntrees, iters, m,
                               RsOut{g.at<uint16_t>(sg), g.at<int64_t>(va), g.at<int64_t>(be), g.at<uint8_t>(su)}, work);
    });
}

int pk_solve_turn_trees_d(int device, size_t m, const uint8_t *board_d, const uint64_t *dead_d, const uint16_t *ranges_d, uint32_t ntrees, const uint32_t *n,
                          const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of_d, uint32_t iters,
                          uint16_t *strategy_d, uint16_t *river_strategy_d, int64_t *value_d, int64_t *br_d, uint8_t *status_d, void *stream) {
    const char *call = "pk_solve_turn_trees_d";
    TsPacked p;
    EQ_REFUSE(g_fail, call, ts_pack_trees(m, board_d && ranges_d && status_d, iters, ntrees, n, kind, child, put, pot, tree_of_d, p));
    const bool solve = strategy_d || river_strategy_d || value_d || br_d;
    const size_t ws = ts_work_bytes(m, p.ntmax, p.nrmax, solve);
    return eq_call_d(call, device, stream, m, EQ_TAB_EVAL, ws + (solve ? ts_trees_bytes(ntrees) : 0), [&](hipStream_t st, const uint32_t *tab, char *work) {
        TsTree *trees_d = (TsTree *)(work + ws);
        if (solve)
            if (const hipError_t e = hipMemcpyAsync(trees_d, p.trees.data(), (size_t)ntrees * sizeof(TsTree), hipMemcpyHostToDevice, st)) return e;
        return ts_launch_trees(st, tab, TsSpots{board_d, dead_d, ranges_d}, TsTrees{trees_d, tree_of_d, p.ntmax, p.nrmax, p.Dtmax, p.Drmax}, ntrees, iters, m,
                               TsOut{strategy_d, river_strategy_d, value_d, br_d, status_d}, work);
    });
}

int pk_solve_turn_trees(int device, size_t m, const uint8_t *board, const uint64_t *dead, const uint16_t *ranges, uint32_t ntrees, const uint32_t *n,
                        const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of, uint32_t iters,
                        uint16_t *strategy, uint16_t *river_strategy, int64_t *value, int64_t *br, uint8_t *status) {
    const char *call = "pk_solve_turn_trees";
    TsPacked p;
    EQ_REFUSE(g_fail, call, ts_pack_trees(m, board && ranges && status, iters, ntrees, n, kind, child, put, pot, tree_of, p));
    const bool solve = strategy || river_strategy || value || br;
    Stage g;
    const int bo = g.in(board, m * 4), de = g.in(dead, m * 8), ra = g.in(ranges, m * 2 * RS_HOLDINGS * 2), to = g.in(tree_of, m * 4);
    const int tr = g.in(solve ? p.trees.data() : nullptr, (size_t)ntrees * sizeof(TsTree));
    const int sg = g.out(strategy, m * p.Dtmax * 4 * RS_HOLDINGS * 2), rg = g.out(river_strategy, m * p.Drmax * 52 * 4 * RS_HOLDINGS * 2);
    const int va = g.out(value, m * 2 * RS_HOLDINGS * 8), be = g.out(br, m * 2 * RS_HOLDINGS * 8), su = g.out(status, m);
    return eq_call_host(call, device, m, EQ_TAB_EVAL, g, ts_work_bytes(m, p.ntmax, p.nrmax, solve), [&](hipStream_t st, const uint32_t *tab, char *work) {
        return ts_launch_trees(st, tab, TsSpots{g.at<uint8_t>(bo), g.at<uint64_t>(de), g.at<uint16_t>(ra)},
                               TsTrees{g.at<TsTree>(tr), g.at<uint32_t>(to), p.ntmax, p.nrmax, p.Dtmax, p.Drmax}, ntrees, iters, m,
                               TsOut{g.at<uint16_t>(sg), g.at<uint16_t>(rg), g.at<int64_t>(va), g.at<int64_t>(be), g.at<uint8_t>(su)}, work);
    });
}

// ---- locked nodes (pokerl_hip.h "Locked nodes"): the tree-per-spot calls with rows of the strategies fixed by the
// caller.  The trees are checked and packed by the code above, with its texts; iters may be 0; tree_of may be NULL with one tree.
static const char *lock_check(uint32_t iters, uint32_t ntrees, const void *tree_of) {
    if (iters > (uint32_t)RS_MAX_ITERS) return ": iters outside 0 .. 4096";
    if (!tree_of && ntrees != 1u) return ": tree_of is NULL with ntrees != 1";
    return nullptr;
}
static const char *lock_pair(const void *lock, const void *locked, const void *out, const char *missing, const char *overlap) {
    if (lock && !locked) return missing;
    if (locked && locked == out) return overlap;
    return nullptr;
}
static const char *rs_lock_pack(size_t m, bool pointers, uint32_t iters, uint32_t ntrees, const uint32_t *n, const uint8_t *kind, const uint8_t *child,
                                const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of, const uint8_t *lock, const uint16_t *locked,
                                const uint16_t *strategy, RsPacked &p) {
    if (const char *why = lock_check(iters, ntrees, tree_of)) return why;
    if (const char *why = lock_pair(lock, locked, strategy, ": lock without locked", ": locked and strategy are the same buffer")) return why;
    // (the existing check refuses 0 iterations and a NULL tree_of: both have been judged above)
    return rs_pack_trees(m, pointers, iters ? iters : 1u, ntrees, n, kind, child, put, pot, tree_of ? tree_of : n, p);
}
static const char *ts_lock_pack(size_t m, bool pointers, uint32_t iters, uint32_t ntrees, const uint32_t *n, const uint8_t *kind, const uint8_t *child,
                                const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of, const uint8_t *lock, const uint16_t *locked,
                                const uint8_t *river_lock, const uint16_t *river_locked, const uint16_t *strategy, const uint16_t *river_strategy,
                                TsPacked &p) {
    if (const char *why = lock_check(iters, ntrees, tree_of)) return why;
    if (const char *why = lock_pair(lock, locked, strategy, ": lock without locked", ": locked and strategy are the same buffer")) return why;
    if (const char *why = lock_pair(river_lock, river_locked, river_strategy, ": river_lock without river_locked",
                                    ": river_locked and river_strategy are the same buffer"))
        return why;
    return ts_pack_trees(m, pointers, iters ? iters : 1u, ntrees, n, kind, child, put, pot, tree_of ? tree_of : n, p);
}

int pk_solve_river_locked_d(int device, size_t m, const uint8_t *board_d, const uint64_t *dead_d, const uint16_t *ranges_d, uint32_t ntrees, const uint32_t *n,
                            const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of_d, uint32_t iters,
                            const uint8_t *lock_d, const uint16_t *locked_d, uint16_t *strategy_d, int64_t *value_d, int64_t *br_d, uint8_t *status_d,
                            void *stream) {
    const char *call = "pk_solve_river_locked_d";
    RsPacked p;
    EQ_REFUSE(g_fail, call, rs_lock_pack(m, board_d && ranges_d && status_d, iters, ntrees, n, kind, child, put, pot, tree_of_d, lock_d, locked_d, strategy_d, p));
    const bool solve = strategy_d || value_d || br_d;
    const size_t ws = rs_work_bytes(m, p.nmax, solve);
    return eq_call_d(call, device, stream, m, EQ_TAB_EVAL, ws + (solve ? rs_trees_bytes(ntrees) : 0), [&](hipStream_t st, const uint32_t *tab, char *work) {
        RsTree *trees_d = (RsTree *)(work + ws);
        if (solve)
            if (const hipError_t e = hipMemcpyAsync(trees_d, p.trees.data(), (size_t)ntrees * sizeof(RsTree), hipMemcpyHostToDevice, st)) return e;
        return rs_launch_locked(st, tab, RsSpots{board_d, dead_d, ranges_d}, RsTrees{trees_d, tree_of_d, p.nmax, p.Dmax}, ntrees, RsLock{lock_d, locked_d},
                                iters, m, RsOut{strategy_d, value_d, br_d, status_d}, work);
    });
}

int pk_solve_river_locked(int device, size_t m, const uint8_t *board, const uint64_t *dead, const uint16_t *ranges, uint32_t ntrees, const uint32_t *n,
                          const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of, uint32_t iters,
                          const uint8_t *lock, const uint16_t *locked, uint16_t *strategy, int64_t *value, int64_t *br, uint8_t *status) {
    const char *call = "pk_solve_river_locked";
    RsPacked p;
    EQ_REFUSE(g_fail, call, rs_lock_pack(m, board && ranges && status, iters, ntrees, n, kind, child, put, pot, tree_of, lock, locked, strategy, p));
    const bool solve = strategy || value || br;
    Stage g;
    const int bo = g.in(board, m * 5), de = g.in(dead, m * 8), ra = g.in(ranges, m * 2 * RS_HOLDINGS * 2), to = g.in(tree_of, m * 4);
    const int tr = g.in(solve ? p.trees.data() : nullptr, (size_t)ntrees * sizeof(RsTree));
    const int lo = g.in(solve ? lock : nullptr, m * p.Dmax), ld = g.in(solve && lock ? locked : nullptr, m * p.Dmax * 4 * RS_HOLDINGS * 2);
    const int sg = g.out(strategy, m * p.Dmax * 4 * RS_HOLDINGS * 2), va = g.out(value, m * 2 * RS_HOLDINGS * 8), be = g.out(br, m * 2 * RS_HOLDINGS * 8);
    const int su = g.out(status, m);
    return eq_call_host(call, device, m, EQ_TAB_EVAL, g, rs_work_bytes(m, p.nmax, solve), [&](hipStream_t st, const uint32_t *tab, char *work) {
        return rs_launch_locked(st, tab, RsSpots{g.at<uint8_t>(bo), g.at<uint64_t>(de), g.at<uint16_t>(ra)},
                                RsTrees{g.at<RsTree>(tr), g.at<uint32_t>(to), p.nmax, p.Dmax}, ntrees, RsLock{g.at<uint8_t>(lo), g.at<uint16_t>(ld)}, iters, m,
                                RsOut{g.at<uint16_t>(sg), g.at<int64_t>(va), g.at<int64_t>(be), g.at<uint8_t>(su)}, work);
    });
}

int pk_solve_turn_locked_d(int device, size_t m, const uint8_t *board_d, const uint64_t *dead_d, const uint16_t *ranges_d, uint32_t ntrees, const uint32_t *n,
                           const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of_d, uint32_t iters,
                           const uint8_t *lock_d, const uint16_t *locked_d, const uint8_t *river_lock_d, const uint16_t *river_locked_d, uint16_t *strategy_d,
                           uint16_t *river_strategy_d, int64_t *value_d, int64_t *br_d, uint8_t *status_d, void *stream) {
    const char *call = "pk_solve_turn_locked_d";
    TsPacked p;
    EQ_REFUSE(g_fail, call, ts_lock_pack(m, board_d && ranges_d && status_d, iters, ntrees, n, kind, child, put, pot, tree_of_d, lock_d, locked_d, river_lock_d,
                                         river_locked_d, strategy_d, river_strategy_d, p));
    const bool solve = strategy_d || river_strategy_d || value_d || br_d;
    const size_t ws = ts_work_bytes(m, p.ntmax, p.nrmax, solve);
    return eq_call_d(call, device, stream, m, EQ_TAB_EVAL, ws + (solve ? ts_trees_bytes(ntrees) : 0), [&](hipStream_t st, const uint32_t *tab, char *work) {
        TsTree *trees_d = (TsTree *)(work + ws);
        if (solve)
            if (const hipError_t e = hipMemcpyAsync(trees_d, p.trees.data(), (size_t)ntrees * sizeof(TsTree), hipMemcpyHostToDevice, st)) return e;
        return ts_launch_locked(st, tab, TsSpots{board_d, dead_d, ranges_d}, TsTrees{trees_d, tree_of_d, p.ntmax, p.nrmax, p.Dtmax, p.Drmax}, ntrees,
                                TsLock{lock_d, locked_d, river_lock_d, river_locked_d}, iters, m,
                                TsOut{strategy_d, river_strategy_d, value_d, br_d, status_d}, work);
    });
}

int pk_solve_turn_locked(int device, size_t m, const uint8_t *board, const uint64_t *dead, const uint16_t *ranges, uint32_t ntrees, const uint32_t *n,
                         const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of, uint32_t iters,
                         const uint8_t *lock, const uint16_t *locked, const uint8_t *river_lock, const uint16_t *river_locked, uint16_t *strategy,
                         uint16_t *river_strategy, int64_t *value, int64_t *br, uint8_t *status) {
    const char *call = "pk_solve_turn_locked";
    TsPacked p;
    EQ_REFUSE(g_fail, call, ts_lock_pack(m, board && ranges && status, iters, ntrees, n, kind, child, put, pot, tree_of, lock, locked, river_lock, river_locked,
                                         strategy, river_strategy, p));
    const bool solve = strategy || river_strategy || value || br;
    Stage g;
    const int bo = g.in(board, m * 4), de = g.in(dead, m * 8), ra = g.in(ranges, m * 2 * RS_HOLDINGS * 2), to = g.in(tree_of, m * 4);
    const int tr = g.in(solve ? p.trees.data() : nullptr, (size_t)ntrees * sizeof(TsTree));
    const int lo = g.in(solve ? lock : nullptr, m * p.Dtmax), ld = g.in(solve && lock ? locked : nullptr, m * p.Dtmax * 4 * RS_HOLDINGS * 2);
    const int ro = g.in(solve ? river_lock : nullptr, m * p.Drmax);
    const int rd = g.in(solve && river_lock ? river_locked : nullptr, m * p.Drmax * 52 * 4 * RS_HOLDINGS * 2);
    const int sg = g.out(strategy, m * p.Dtmax * 4 * RS_HOLDINGS * 2), rg = g.out(river_strategy, m * p.Drmax * 52 * 4 * RS_HOLDINGS * 2);
    const int va = g.out(value, m * 2 * RS_HOLDINGS * 8), be = g.out(br, m * 2 * RS_HOLDINGS * 8), su = g.out(status, m);
    return eq_call_host(call, device, m, EQ_TAB_EVAL, g, ts_work_bytes(m, p.ntmax, p.nrmax, solve), [&](hipStream_t st, const uint32_t *tab, char *work) {
        return ts_launch_locked(st, tab, TsSpots{g.at<uint8_t>(bo), g.at<uint64_t>(de), g.at<uint16_t>(ra)},
                                TsTrees{g.at<TsTree>(tr), g.at<uint32_t>(to), p.ntmax, p.nrmax, p.Dtmax, p.Drmax}, ntrees,
                                TsLock{g.at<uint8_t>(lo), g.at<uint16_t>(ld), g.at<uint8_t>(ro), g.at<uint16_t>(rd)}, iters, m,
                                TsOut{g.at<uint16_t>(sg), g.at<uint16_t>(rg), g.at<int64_t>(va), g.at<int64_t>(be), g.at<uint8_t>(su)}, work);
    });
}

// ---- re-solving (pokerl_hip.h "Re-solving"): the locked calls with root reaches in the solver's own units, a terminal
// of given values (river) and the reaches, values and best-response values at one node of each spot's tree.
static const char *resolve_check(const void *reach, const void *given, const void *at, const void *node_reach, const void *node_value, const void *node_br,
                                 const void *value, const void *br) {
    if ((at != nullptr) != (node_reach || node_value || node_br)) return ": at comes with node_reach, node_value or node_br, and only with one of them";
    if (reach && reach == node_reach) return ": reach and node_reach are the same buffer";
    if (given && (given == value || given == br || given == node_value || given == node_br)) return ": given and an output are the same buffer";
    return nullptr;
}
static const char *rs_resolve_pack(size_t m, const uint8_t *board, const uint16_t *ranges, const uint8_t *status, uint32_t iters, uint32_t ntrees, const uint32_t *n,
                                   const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of, const uint8_t *lock,
                                   const uint16_t *locked, const RsResolve &rz, const RsOut &out, RsPacked &p) {
    if (const char *why = lock_check(iters, ntrees, tree_of)) return why;
    if (const char *why = lock_pair(lock, locked, out.strategy, ": lock without locked", ": locked and strategy are the same buffer")) return why;
    if (const char *why = resolve_check(rz.reach, rz.given, rz.at, rz.node_reach, rz.node_value, rz.node_br, out.value, out.br)) return why;
    if (const char *why = rs_pack_trees(m, board && (ranges || rz.reach) && status, iters ? iters : 1u, ntrees, n, kind, child, put, pot, tree_of ? tree_of : n, p, true))
        return why;
    if (p.given && !rz.given) return ": a tree has a given node and given is NULL";
    return nullptr;
}
static const char *ts_resolve_pack(size_t m, const uint8_t *board, const uint16_t *ranges, const uint8_t *status, uint32_t iters, uint32_t ntrees, const uint32_t *n,
                                   const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of, const TsLock &lk,
                                   const TsResolve &rz, const TsOut &out, TsPacked &p) {
    if (const char *why = lock_check(iters, ntrees, tree_of)) return why;
    if (const char *why = lock_pair(lk.lock, lk.locked, out.strategy, ": lock without locked", ": locked and strategy are the same buffer")) return why;
    if (const char *why = lock_pair(lk.river_lock, lk.river_locked, out.river_strategy, ": river_lock without river_locked",
                                    ": river_locked and river_strategy are the same buffer"))
        return why;
    if (const char *why = resolve_check(rz.reach, nullptr, rz.at, rz.node_reach, rz.node_value, rz.node_br, out.value, out.br)) return why;
    return ts_pack_trees(m, board && (ranges || rz.reach) && status, iters ? iters : 1u, ntrees, n, kind, child, put, pot, tree_of ? tree_of : n, p);
}

int pk_solve_river_resolve_d(int device, size_t m, const uint8_t *board_d, const uint64_t *dead_d, const uint16_t *ranges_d, uint32_t ntrees, const uint32_t *n,
                             const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of_d, uint32_t iters,
                             const uint8_t *lock_d, const uint16_t *locked_d, const uint32_t *reach_d, const int64_t *given_d, const uint8_t *at_d,
                             uint16_t *strategy_d, int64_t *value_d, int64_t *br_d, uint32_t *node_reach_d, int64_t *node_value_d, int64_t *node_br_d,
                             uint8_t *status_d, void *stream) {
    const char *call = "pk_solve_river_resolve_d";
    RsPacked p;
    const RsResolve rz{reach_d, given_d, at_d, node_reach_d, node_value_d, node_br_d};
    const RsOut out{strategy_d, value_d, br_d, status_d};
    EQ_REFUSE(g_fail, call, rs_resolve_pack(m, board_d, ranges_d, status_d, iters, ntrees, n, kind, child, put, pot, tree_of_d, lock_d, locked_d, rz, out, p));
    const bool solve = strategy_d || value_d || br_d || at_d;
    const size_t ws = rs_work_bytes(m, p.nmax, solve);
    return eq_call_d(call, device, stream, m, EQ_TAB_EVAL, ws + (solve ? rs_trees_bytes(ntrees) : 0), [&](hipStream_t st, const uint32_t *tab, char *work) {
        RsTree *trees_d = (RsTree *)(work + ws);
        if (solve)
            if (const hipError_t e = hipMemcpyAsync(trees_d, p.trees.data(), (size_t)ntrees * sizeof(RsTree), hipMemcpyHostToDevice, st)) return e;
        return rs_launch_resolve(st, tab, RsSpots{board_d, dead_d, ranges_d}, RsTrees{trees_d, tree_of_d, p.nmax, p.Dmax}, ntrees, RsLock{lock_d, locked_d}, rz,
                                 iters, m, out, work);
    });
}

int pk_solve_river_resolve(int device, size_t m, const uint8_t *board, const uint64_t *dead, const uint16_t *ranges, uint32_t ntrees, const uint32_t *n,
                           const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of, uint32_t iters,
                           const uint8_t *lock, const uint16_t *locked, const uint32_t *reach, const int64_t *given, const uint8_t *at, uint16_t *strategy,
                           int64_t *value, int64_t *br, uint32_t *node_reach, int64_t *node_value, int64_t *node_br, uint8_t *status) {
    const char *call = "pk_solve_river_resolve";
    RsPacked p;
    EQ_REFUSE(g_fail, call, rs_resolve_pack(m, board, ranges, status, iters, ntrees, n, kind, child, put, pot, tree_of, lock, locked,
                                            RsResolve{reach, given, at, node_reach, node_value, node_br}, RsOut{strategy, value, br, status}, p));
    const bool solve = strategy || value || br || at;
    const size_t row = m * 2 * RS_HOLDINGS;
    Stage g;
    const int bo = g.in(board, m * 5), de = g.in(dead, m * 8), ra = g.in(reach ? nullptr : ranges, row * 2), to = g.in(tree_of, m * 4);
    const int tr = g.in(solve ? p.trees.data() : nullptr, (size_t)ntrees * sizeof(RsTree));
    const int lo = g.in(solve ? lock : nullptr, m * p.Dmax), ld = g.in(solve && lock ? locked : nullptr, m * p.Dmax * 4 * RS_HOLDINGS * 2);
    const int re = g.in(solve ? reach : nullptr, row * 4), gi = g.in(solve && p.given ? given : nullptr, row * 8), an = g.in(at, m);
    const int sg = g.out(strategy, m * p.Dmax * 4 * RS_HOLDINGS * 2), va = g.out(value, row * 8), be = g.out(br, row * 8);
    const int nr = g.out(node_reach, row * 4), nv = g.out(node_value, row * 8), nb = g.out(node_br, row * 8), su = g.out(status, m);
    return eq_call_host(call, device, m, EQ_TAB_EVAL, g, rs_work_bytes(m, p.nmax, solve), [&](hipStream_t st, const uint32_t *tab, char *work) {
        return rs_launch_resolve(st, tab, RsSpots{g.at<uint8_t>(bo), g.at<uint64_t>(de), g.at<uint16_t>(ra)},
                                 RsTrees{g.at<RsTree>(tr), g.at<uint32_t>(to), p.nmax, p.Dmax}, ntrees, RsLock{g.at<uint8_t>(lo), g.at<uint16_t>(ld)},
                                 RsResolve{g.at<uint32_t>(re), g.at<int64_t>(gi), g.at<uint8_t>(an), g.at<uint32_t>(nr), g.at<int64_t>(nv), g.at<int64_t>(nb)},
                                 iters, m, RsOut{g.at<uint16_t>(sg), g.at<int64_t>(va), g.at<int64_t>(be), g.at<uint8_t>(su)}, work);
    });
}

int pk_solve_turn_resolve_d(int device, size_t m, const uint8_t *board_d, const uint64_t *dead_d, const uint16_t *ranges_d, uint32_t ntrees, const uint32_t *n,
                            const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of_d, uint32_t iters,
                            const uint8_t *lock_d, const uint16_t *locked_d, const uint8_t *river_lock_d, const uint16_t *river_locked_d, const uint32_t *reach_d,
                            const uint8_t *at_d, const uint8_t *at_card_d, uint16_t *strategy_d, uint16_t *river_strategy_d, int64_t *value_d, int64_t *br_d,
                            uint32_t *node_reach_d, int64_t *node_value_d, int64_t *node_br_d, uint8_t *status_d, void *stream) {
    const char *call = "pk_solve_turn_resolve_d";
    TsPacked p;
    const TsLock lk{lock_d, locked_d, river_lock_d, river_locked_d};
    const TsResolve rz{reach_d, at_d, at_card_d, node_reach_d, node_value_d, node_br_d};
    const TsOut out{strategy_d, river_strategy_d, value_d, br_d, status_d};
    EQ_REFUSE(g_fail, call, ts_resolve_pack(m, board_d, ranges_d, status_d, iters, ntrees, n, kind, child, put, pot, tree_of_d, lk, rz, out, p));
    const bool solve = strategy_d || river_strategy_d || value_d || br_d || at_d;
    const size_t ws = ts_work_bytes(m, p.ntmax, p.nrmax, solve);
    return eq_call_d(call, device, stream, m, EQ_TAB_EVAL, ws + (solve ? ts_trees_bytes(ntrees) : 0), [&](hipStream_t st, const uint32_t *tab, char *work) {
        TsTree *trees_d = (TsTree *)(work + ws);
        if (solve)
            if (const hipError_t e = hipMemcpyAsync(trees_d, p.trees.data(), (size_t)ntrees * sizeof(TsTree), hipMemcpyHostToDevice, st)) return e;
        return ts_launch_resolve(st, tab, TsSpots{board_d, dead_d, ranges_d}, TsTrees{trees_d, tree_of_d, p.ntmax, p.nrmax, p.Dtmax, p.Drmax}, ntrees, lk, rz, iters,
                                 m, out, work);
    });
}

int pk_solve_turn_resolve(int device, size_t m, const uint8_t *board, const uint64_t *dead, const uint16_t *ranges, uint32_t ntrees, const uint32_t *n,
                          const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of, uint32_t iters,
                          const uint8_t *lock, const uint16_t *locked, const uint8_t *river_lock, const uint16_t *river_locked, const uint32_t *reach,
                          const uint8_t *at, const uint8_t *at_card, uint16_t *strategy, uint16_t *river_strategy, int64_t *value, int64_t *br,
                          uint32_t *node_reach, int64_t *node_value, int64_t *node_br, uint8_t *status) {
    const char *call = "pk_solve_turn_resolve";
    TsPacked p;
    EQ_REFUSE(g_fail, call, ts_resolve_pack(m, board, ranges, status, iters, ntrees, n, kind, child, put, pot, tree_of, TsLock{lock, locked, river_lock, river_locked},
                                            TsResolve{reach, at, at_card, node_reach, node_value, node_br}, TsOut{strategy, river_strategy, value, br, status}, p));
    const bool solve = strategy || river_strategy || value || br || at;
    const size_t row = m * 2 * RS_HOLDINGS;
    Stage g;
    const int bo = g.in(board, m * 4), de = g.in(dead, m * 8), ra = g.in(reach ? nullptr : ranges, row * 2), to = g.in(tree_of, m * 4);
    const int tr = g.in(solve ? p.trees.data() : nullptr, (size_t)ntrees * sizeof(TsTree));
    const int lo = g.in(solve ? lock : nullptr, m * p.Dtmax), ld = g.in(solve && lock ? locked : nullptr, m * p.Dtmax * 4 * RS_HOLDINGS * 2);
    const int ro = g.in(solve ? river_lock : nullptr, m * p.Drmax);
    const int rd = g.in(solve && river_lock ? river_locked : nullptr, m * p.Drmax * 52 * 4 * RS_HOLDINGS * 2);
    const int re = g.in(solve ? reach : nullptr, row * 4), an = g.in(at, m), ac = g.in(at ? at_card : nullptr, m);
    const int sg = g.out(strategy, m * p.Dtmax * 4 * RS_HOLDINGS * 2), rg = g.out(river_strategy, m * p.Drmax * 52 * 4 * RS_HOLDINGS * 2);
    const int va = g.out(value, row * 8), be = g.out(br, row * 8);
    const int nr = g.out(node_reach, row * 4), nv = g.out(node_value, row * 8), nb = g.out(node_br, row * 8), su = g.out(status, m);
    return eq_call_host(call, device, m, EQ_TAB_EVAL, g, ts_work_bytes(m, p.ntmax, p.nrmax, solve), [&](hipStream_t st, const uint32_t *tab, char *work) {
        return ts_launch_resolve(st, tab, TsSpots{g.at<uint8_t>(bo), g.at<uint64_t>(de), g.at<uint16_t>(ra)},
                                 TsTrees{g.at<TsTree>(tr), g.at<uint32_t>(to), p.ntmax, p.nrmax, p.Dtmax, p.Drmax}, ntrees,
                                 TsLock{g.at<uint8_t>(lo), g.at<uint16_t>(ld), g.at<uint8_t>(ro), g.at<uint16_t>(rd)},
                                 TsResolve{g.at<uint32_t>(re), g.at<uint8_t>(an), g.at<uint8_t>(ac), g.at<uint32_t>(nr), g.at<int64_t>(nv), g.at<int64_t>(nb)}, iters, m,
                                 TsOut{g.at<uint16_t>(sg), g.at<uint16_t>(rg), g.at<int64_t>(va), g.at<int64_t>(be), g.at<uint8_t>(su)}, work);
    });
}

// ---- resuming (pokerl_hip.h "Resuming a solve"): the re-solving call with the regrets and the average accumulators in
// the caller's memory, in and out, and the iterations they hold.  Without state the call is the re-solving call.
// (state: the call's state arrays -- two on the river, four on the turn; others: every other array of the call)
static const char *resume_check(const void *t0, std::initializer_list<const void *> state, std::initializer_list<const void *> others, const char *together,
                                const char *alone) {
    size_t given = 0;
    for (const void *a : state) given += a ? 1u : 0u;
    if (given && given != state.size()) return together;
    if (t0 && !given) return alone;
    for (const void *a : state) {
        if (!a) continue;
        size_t same = 0;
        for (const void *b : state) same += a == b ? 1u : 0u;
        if (same != 1u || a == t0) return ": a state array is another argument of the call";
        for (const void *o : others)
            if (o == a) return ": a state array is another argument of the call";
    }
    return nullptr;
}

int pk_solve_river_resume_d(int device, size_t m, const uint8_t *board_d, const uint64_t *dead_d, const uint16_t *ranges_d, uint32_t ntrees, const uint32_t *n,
                            const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of_d, uint32_t iters,
                            const uint8_t *lock_d, const uint16_t *locked_d, const uint32_t *reach_d, const int64_t *given_d, const uint8_t *at_d,
                            const uint32_t *t0_d, int64_t *regret_d, int64_t *average_d, uint16_t *strategy_d, int64_t *value_d, int64_t *br_d,
                            uint32_t *node_reach_d, int64_t *node_value_d, int64_t *node_br_d, uint8_t *status_d, void *stream) {
    const char *call = "pk_solve_river_resume_d";
    EQ_REFUSE(g_fail, call, resume_check(t0_d, {regret_d, average_d}, {board_d, dead_d, ranges_d, tree_of_d, lock_d, locked_d, reach_d, given_d, at_d, strategy_d,
                                                                       value_d, br_d, node_reach_d, node_value_d, node_br_d, status_d},
                                         ": regret and average come together", ": t0 without regret and average"));
    if (!regret_d)
        return pk_solve_river_resolve_d(device, m, board_d, dead_d, ranges_d, ntrees, n, kind, child, put, pot, tree_of_d, iters, lock_d, locked_d, reach_d,
                                        given_d, at_d, strategy_d, value_d, br_d, node_reach_d, node_value_d, node_br_d, status_d, stream);
    RsPacked p;
    const RsResolve rz{reach_d, given_d, at_d, node_reach_d, node_value_d, node_br_d};
    const RsOut out{strategy_d, value_d, br_d, status_d};
    EQ_REFUSE(g_fail, call, rs_resolve_pack(m, board_d, ranges_d, status_d, iters, ntrees, n, kind, child, put, pot, tree_of_d, lock_d, locked_d, rz, out, p));
    const size_t ws = rs_work_bytes(m, p.nmax, true);
    return eq_call_d(call, device, stream, m, EQ_TAB_EVAL, ws + rs_trees_bytes(ntrees), [&](hipStream_t st, const uint32_t *tab, char *work) {
        RsTree *trees_d = (RsTree *)(work + ws);
        if (const hipError_t e = hipMemcpyAsync(trees_d, p.trees.data(), (size_t)ntrees * sizeof(RsTree), hipMemcpyHostToDevice, st)) return e;
        return rs_launch_resume(st, tab, RsSpots{board_d, dead_d, ranges_d}, RsTrees{trees_d, tree_of_d, p.nmax, p.Dmax}, ntrees, RsLock{lock_d, locked_d}, rz,
                                RsResume{t0_d, regret_d, average_d}, iters, m, out, work);
    });
}

int pk_solve_river_resume(int device, size_t m, const uint8_t *board, const uint64_t *dead, const uint16_t *ranges, uint32_t ntrees, const uint32_t *n,
                          const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of, uint32_t iters,
                          const uint8_t *lock, const uint16_t *locked, const uint32_t *reach, const int64_t *given, const uint8_t *at, const uint32_t *t0,
                          int64_t *regret, int64_t *average, uint16_t *strategy, int64_t *value, int64_t *br, uint32_t *node_reach, int64_t *node_value,
                          int64_t *node_br, uint8_t *status) {
    const char *call = "pk_solve_river_resume";
    EQ_REFUSE(g_fail, call, resume_check(t0, {regret, average}, {board, dead, ranges, tree_of, lock, locked, reach, given, at, strategy, value, br, node_reach,
                                                                 node_value, node_br, status},
                                         ": regret and average come together", ": t0 without regret and average"));
    if (!regret)
        return pk_solve_river_resolve(device, m, board, dead, ranges, ntrees, n, kind, child, put, pot, tree_of, iters, lock, locked, reach, given, at, strategy,
                                      value, br, node_reach, node_value, node_br, status);
    RsPacked p;
    EQ_REFUSE(g_fail, call, rs_resolve_pack(m, board, ranges, status, iters, ntrees, n, kind, child, put, pot, tree_of, lock, locked,
                                            RsResolve{reach, given, at, node_reach, node_value, node_br}, RsOut{strategy, value, br, status}, p));
    const size_t row = m * 2 * RS_HOLDINGS, rows = m * p.Dmax * 4 * RS_HOLDINGS;
    Stage g;
    const int bo = g.in(board, m * 5), de = g.in(dead, m * 8), ra = g.in(reach ? nullptr : ranges, row * 2), to = g.in(tree_of, m * 4);
    const int tr = g.in(p.trees.data(), (size_t)ntrees * sizeof(RsTree));
    const int lo = g.in(lock, m * p.Dmax), ld = g.in(lock ? locked : nullptr, rows * 2);
    const int re = g.in(reach, row * 4), gi = g.in(p.given ? given : nullptr, row * 8), an = g.in(at, m);
    const int tz = g.in(t0, m * 4), rg = g.inout(regret, rows * 8), av = g.inout(average, rows * 8);
    const int sg = g.out(strategy, rows * 2), va = g.out(value, row * 8), be = g.out(br, row * 8);
    const int nr = g.out(node_reach, row * 4), nv = g.out(node_value, row * 8), nb = g.out(node_br, row * 8), su = g.out(status, m);
    return eq_call_host(call, device, m, EQ_TAB_EVAL, g, rs_work_bytes(m, p.nmax, true), [&](hipStream_t st, const uint32_t *tab, char *work) {
        return rs_launch_resume(st, tab, RsSpots{g.at<uint8_t>(bo), g.at<uint64_t>(de), g.at<uint16_t>(ra)},
                                RsTrees{g.at<RsTree>(tr), g.at<uint32_t>(to), p.nmax, p.Dmax}, ntrees, RsLock{g.at<uint8_t>(lo), g.at<uint16_t>(ld)},
                                RsResolve{g.at<uint32_t>(re), g.at<int64_t>(gi), g.at<uint8_t>(an), g.at<uint32_t>(nr), g.at<int64_t>(nv), g.at<int64_t>(nb)},
                                RsResume{g.at<uint32_t>(tz), g.at<int64_t>(rg), g.at<int64_t>(av)}, iters, m,
                                RsOut{g.at<uint16_t>(sg), g.at<int64_t>(va), g.at<int64_t>(be), g.at<uint8_t>(su)}, work);
    });
}

static const char *const TS_STATE_TOGETHER = ": regret, average, river_regret and river_average come together";
static const char *const TS_STATE_ALONE = ": t0 without regret, average, river_regret and river_average";

int pk_solve_turn_resume_d(int device, size_t m, const uint8_t *board_d, const uint64_t *dead_d, const uint16_t *ranges_d, uint32_t ntrees, const uint32_t *n,
                           const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of_d, uint32_t iters,
                           const uint8_t *lock_d, const uint16_t *locked_d, const uint8_t *river_lock_d, const uint16_t *river_locked_d, const uint32_t *reach_d,
                           const uint8_t *at_d, const uint8_t *at_card_d, const uint32_t *t0_d, int64_t *regret_d, int64_t *average_d, int64_t *river_regret_d,
                           int64_t *river_average_d, uint16_t *strategy_d, uint16_t *river_strategy_d, int64_t *value_d, int64_t *br_d, uint32_t *node_reach_d,
                           int64_t *node_value_d, int64_t *node_br_d, uint8_t *status_d, void *stream) {
    const char *call = "pk_solve_turn_resume_d";
    EQ_REFUSE(g_fail, call, resume_check(t0_d, {regret_d, average_d, river_regret_d, river_average_d},
                                         {board_d, dead_d, ranges_d, tree_of_d, lock_d, locked_d, river_lock_d, river_locked_d, reach_d, at_d, at_card_d, strategy_d,
                                          river_strategy_d, value_d, br_d, node_reach_d, node_value_d, node_br_d, status_d},
                                         TS_STATE_TOGETHER, TS_STATE_ALONE));
    if (!regret_d)
        return pk_solve_turn_resolve_d(device, m, board_d, dead_d, ranges_d, ntrees, n, kind, child, put, pot, tree_of_d, iters, lock_d, locked_d, river_lock_d,
                                       river_locked_d, reach_d, at_d, at_card_d, strategy_d, river_strategy_d, value_d, br_d, node_reach_d, node_value_d, node_br_d,
                                       status_d, stream);
    TsPacked p;
    const TsLock lk{lock_d, locked_d, river_lock_d, river_locked_d};
    const TsResolve rz{reach_d, at_d, at_card_d, node_reach_d, node_value_d, node_br_d};
    const TsOut out{strategy_d, river_strategy_d, value_d, br_d, status_d};
    EQ_REFUSE(g_fail, call, ts_resolve_pack(m, board_d, ranges_d, status_d, iters, ntrees, n, kind, child, put, pot, tree_of_d, lk, rz, out, p));
    const size_t ws = ts_work_bytes(m, p.ntmax, p.nrmax, true);
    return eq_call_d(call, device, stream, m, EQ_TAB_EVAL, ws + ts_trees_bytes(ntrees), [&](hipStream_t st, const uint32_t *tab, char *work) {
        TsTree *trees_d = (TsTree *)(work + ws);
        if (const hipError_t e = hipMemcpyAsync(trees_d, p.trees.data(), (size_t)ntrees * sizeof(TsTree), hipMemcpyHostToDevice, st)) return e;
        return ts_launch_resume(st, tab, TsSpots{board_d, dead_d, ranges_d}, TsTrees{trees_d, tree_of_d, p.ntmax, p.nrmax, p.Dtmax, p.Drmax}, ntrees, lk, rz,
                                TsResume{t0_d, regret_d, average_d, river_regret_d, river_average_d}, iters, m, out, work);
    });
}

int pk_solve_turn_resume(int device, size_t m, const uint8_t *board, const uint64_t *dead, const uint16_t *ranges, uint32_t ntrees, const uint32_t *n,
                         const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of, uint32_t iters,
                         const uint8_t *lock, const uint16_t *locked, const uint8_t *river_lock, const uint16_t *river_locked, const uint32_t *reach,
                         const uint8_t *at, const uint8_t *at_card, const uint32_t *t0, int64_t *regret, int64_t *average, int64_t *river_regret,
                         int64_t *river_average, uint16_t *strategy, uint16_t *river_strategy, int64_t *value, int64_t *br, uint32_t *node_reach,
                         int64_t *node_value, int64_t *node_br, uint8_t *status) {
    const char *call = "pk_solve_turn_resume";
    EQ_REFUSE(g_fail, call, resume_check(t0, {regret, average, river_regret, river_average},
                                         {board, dead, ranges, tree_of, lock, locked, river_lock, river_locked, reach, at, at_card, strategy, river_strategy, value, br,
                                          node_reach, node_value, node_br, status},
                                         TS_STATE_TOGETHER, TS_STATE_ALONE));
    if (!regret)
        return pk_solve_turn_resolve(device, m, board, dead, ranges, ntrees, n, kind, child, put, pot, tree_of, iters, lock, locked, river_lock, river_locked, reach, at,
                                     at_card, strategy, river_strategy, value, br, node_reach, node_value, node_br, status);
    TsPacked p;
    EQ_REFUSE(g_fail, call, ts_resolve_pack(m, board, ranges, status, iters, ntrees, n, kind, child, put, pot, tree_of, TsLock{lock, locked, river_lock, river_locked},
                                            TsResolve{reach, at, at_card, node_reach, node_value, node_br}, TsOut{strategy, river_strategy, value, br, status}, p));
    const size_t row = m * 2 * RS_HOLDINGS, trows = m * p.Dtmax * 4 * RS_HOLDINGS, rrows = m * p.Drmax * 52 * 4 * RS_HOLDINGS;
    Stage g;
    const int bo = g.in(board, m * 4), de = g.in(dead, m * 8), ra = g.in(reach ? nullptr : ranges, row * 2), to = g.in(tree_of, m * 4);
    const int tr = g.in(p.trees.data(), (size_t)ntrees * sizeof(TsTree));
    const int lo = g.in(lock, m * p.Dtmax), ld = g.in(lock ? locked : nullptr, trows * 2);
    const int ro = g.in(river_lock, m * p.Drmax), rd = g.in(river_lock ? river_locked : nullptr, rrows * 2);
    const int re = g.in(reach, row * 4), an = g.in(at, m), ac = g.in(at ? at_card : nullptr, m);
    const int tz = g.in(t0, m * 4), rg = g.inout(regret, trows * 8), av = g.inout(average, trows * 8);
    const int rrg = g.inout(river_regret, rrows * 8), rav = g.inout(river_average, rrows * 8);
    const int sg = g.out(strategy, trows * 2), rs = g.out(river_strategy, rrows * 2);
    const int va = g.out(value, row * 8), be = g.out(br, row * 8);
    const int nr = g.out(node_reach, row * 4), nv = g.out(node_value, row * 8), nb = g.out(node_br, row * 8), su = g.out(status, m);
    return eq_call_host(call, device, m, EQ_TAB_EVAL, g, ts_work_bytes(m, p.ntmax, p.nrmax, true), [&](hipStream_t st, const uint32_t *tab, char *work) {
        return ts_launch_resume(st, tab, TsSpots{g.at<uint8_t>(bo), g.at<uint64_t>(de), g.at<uint16_t>(ra)},
                                TsTrees{g.at<TsTree>(tr), g.at<uint32_t>(to), p.ntmax, p.nrmax, p.Dtmax, p.Drmax}, ntrees,
                                TsLock{g.at<uint8_t>(lo), g.at<uint16_t>(ld), g.at<uint8_t>(ro), g.at<uint16_t>(rd)},
                                TsResolve{g.at<uint32_t>(re), g.at<uint8_t>(an), g.at<uint8_t>(ac), g.at<uint32_t>(nr), g.at<int64_t>(nv), g.at<int64_t>(nb)},
                                TsResume{g.at<uint32_t>(tz), g.at<int64_t>(rg), g.at<int64_t>(av), g.at<int64_t>(rrg), g.at<int64_t>(rav)}, iters, m,
                                TsOut{g.at<uint16_t>(sg), g.at<uint16_t>(rs), g.at<int64_t>(va), g.at<int64_t>(be), g.at<uint8_t>(su)}, work);
    });
}

// ---- the pre-flop solver (pokerl_hip.h "Pre-flop solver"; kernel: pk_preflop_solver.hip).  The trees are the river
// solver's, checked and packed with its check after the two kinds that mean something elsewhere have been refused by name; they go to the
// device as the tree-per-spot calls send them.  tree_of may be NULL (every spot: tree 0).  The table is the resident matchup table.
static const char *ps_pack_trees(size_t m, bool pointers, uint32_t iters, uint32_t ntrees, const uint32_t *n, const uint8_t *kind, const uint8_t *child,
                                 const uint32_t *put, const uint32_t *pot, RsPacked &p) {
    if (const char *why = eq_bad_m(m)) return why;
    if ((m && !pointers) || !n || !kind || !child || !put || !pot) return ": NULL where a pointer is required (ranges, n, kind, child, put, pot, status)";
    if (iters < 1u || iters > (uint32_t)RS_MAX_ITERS) return ": iters outside 1 .. 4096";
    if (ntrees < 1u || ntrees > RS_MAX_TREES) return ": ntrees outside 1 .. 65536";
    p.trees.resize(ntrees);
    for (uint32_t k = 0; k < ntrees; ++k) {
        const size_t row = (size_t)k * RS_MAX_NODES;
        for (uint32_t v = 0; v < n[k] && v < (uint32_t)RS_MAX_NODES; ++v) {
            if (kind[row + v] == TS_CHANCE) return trees_refusal(p.why, k, ": a chance node (kind 5): a pre-flop tree has no later street, a call is a showdown");
            if (kind[row + v] == RS_GIVEN) return trees_refusal(p.why, k, ": a given node (kind 6): the pre-flop solver does not re-solve");
        }
        if (const char *why = rs_check_tree(n[k], kind + row, child + row * 4, put + row * 2, pot[k], p.trees[k])) return trees_refusal(p.why, k, why);
        uint32_t D = 0;
        for (uint32_t v = 0; v < n[k]; ++v) D += p.trees[k].kind[v] <= RS_P1;
        p.nmax = n[k] > p.nmax ? n[k] : p.nmax;
        p.Dmax = D > p.Dmax ? D : p.Dmax;
    }
    return nullptr;
}

int pk_solve_preflop_d(int device, size_t m, const uint16_t *ranges_d, uint32_t ntrees, const uint32_t *n, const uint8_t *kind, const uint8_t *child,
                       const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of_d, uint32_t iters, uint16_t *strategy_d, int64_t *value_d, int64_t *br_d,
                       uint8_t *status_d, void *stream) {
    const char *call = "pk_solve_preflop_d";
    RsPacked p;
    EQ_REFUSE(g_fail, call, ps_pack_trees(m, ranges_d && status_d, iters, ntrees, n, kind, child, put, pot, p));
    const bool solve = strategy_d || value_d || br_d;
    const size_t ws = (ps_work_bytes(m, p.nmax, solve) + 255) & ~(size_t)255;
    return eq_call_d(call, device, stream, m, solve ? EQ_TAB_PREFLOP : EQ_TAB_NONE, ws + rs_trees_bytes(ntrees), [&](hipStream_t st, const uint32_t *M, char *work) {
        RsTree *trees_d = (RsTree *)(work + ws);
        if (const hipError_t e = hipMemcpyAsync(trees_d, p.trees.data(), (size_t)ntrees * sizeof(RsTree), hipMemcpyHostToDevice, st)) return e;
        return ps_launch(st, M, ranges_d, RsTrees{trees_d, tree_of_d, p.nmax, p.Dmax}, ntrees, iters, m, RsOut{strategy_d, value_d, br_d, status_d}, work);
    });
}

int pk_solve_preflop(int device, size_t m, const uint16_t *ranges, uint32_t ntrees, const uint32_t *n, const uint8_t *kind, const uint8_t *child,
                     const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of, uint32_t iters, uint16_t *strategy, int64_t *value, int64_t *br,
                     uint8_t *status) {
    const char *call = "pk_solve_preflop";
    RsPacked p;
    EQ_REFUSE(g_fail, call, ps_pack_trees(m, ranges && status, iters, ntrees, n, kind, child, put, pot, p));
    const bool solve = strategy || value || br;
    Stage g;
    const int ra = g.in(ranges, m * 2 * RS_HOLDINGS * 2), to = g.in(tree_of, m * 4), tr = g.in(p.trees.data(), (size_t)ntrees * sizeof(RsTree));
    const int sg = g.out(strategy, m * p.Dmax * 4 * RS_HOLDINGS * 2), va = g.out(value, m * 2 * RS_HOLDINGS * 8), be = g.out(br, m * 2 * RS_HOLDINGS * 8);
    const int su = g.out(status, m);
    return eq_call_host(call, device, m, solve ? EQ_TAB_PREFLOP : EQ_TAB_NONE, g, ps_work_bytes(m, p.nmax, solve), [&](hipStream_t st, const uint32_t *M, char *work) {
        return ps_launch(st, M, g.at<uint16_t>(ra), RsTrees{g.at<RsTree>(tr), g.at<uint32_t>(to), p.nmax, p.Dmax}, ntrees, iters, m,
                         RsOut{g.at<uint16_t>(sg), g.at<int64_t>(va), g.at<int64_t>(be), g.at<uint8_t>(su)}, work);
    });
}

}  // extern "C"
