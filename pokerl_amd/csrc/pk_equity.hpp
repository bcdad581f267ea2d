// pk_equity.hpp -- showdown equity by exhaustive board enumeration (include/pokerl_hip.h "Showdown equity"): what the
// host entry points (pk_api.hip) and the kernels (pk_equity.hip) share, and the device pieces k_equity<N> shares with k_ev<N>
// (pk_equity_ev.hip).  The existing table kernels do not include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pk_device.hpp"
#include "pk_equity_common.hpp"

namespace pk {

constexpr uint32_t EQ_SHARE_UNIT = PK_EQ_SHARE_UNIT;   // lcm(1 .. 16): a board's pot share of one of nw winners is EQ_SHARE_UNIT / nw, exactly
constexpr int EQ_BLOCK = 512, EQ_WAVES = EQ_BLOCK / 64;
constexpr int EQ_GRID_MAX = 1024;                       // persistent grid: four 512-thread workgroups per CU (4 x 36 KB of LDS)
constexpr int EQ_LPT_MAX = 4096;                        // boards per lane and task at most: a lane's share sum is 32 bits wide
static_assert((uint64_t)EQ_LPT_MAX * EQ_SHARE_UNIT < (1ull << 32), "a lane's 32-bit share sum must hold EQ_LPT_MAX boards of a sole winner");

// Work space of one call, laid out by eq_layout: the control block, one descriptor per spot, the task list.
struct EqCtrl { uint32_t ntasks, next, pad[62]; };
// A spot's descriptor: 3 + N 64-bit words.
//   [0] known board cards, [3 + p] seat p's hole cards: suit-lane bit sets OR(4 << Card.value), what eval7_tab_front_bits takes
//   [1] the pool: bit c set = the card of canonical index c (rank0 * 4 + suit) is not dead
//   [2] boards | live << 32 | k << 48 | P << 56   (k = 5 - nb cards to come, P = cards in the pool; boards = 0 for a refused spot)
struct EqWork {
    EqCtrl *ctrl;
    uint64_t *desc;
    uint2 *tasks;        // (spot, chunk): one wavefront's share of a spot's boards
    size_t task_cap;
};
// One description of the work space, run with base == NULL to measure it.  pool_max: the largest pool a spot of the call can have (the
// explicit form: 50, a live seat holds two known cards; the table form: 52 - 2N) -- it bounds the task list, C(pool_max, 5) boards per spot.
size_t eq_layout(int N, size_t m, int lpt, int pool_max, char *base, EqWork *w);
// Slots of the task list eq_layout reserves: m * ceil(C(pool_max, 5) / (64 * lpt)).  The task count is a 32-bit word on the device, so
// the entry points refuse a call whose bound does not fit (PK_E_INVALID_ARG) instead of letting it wrap.
size_t eq_task_cap(size_t m, int lpt, int pool_max);
constexpr size_t EQ_TASKS_MAX = 0xFFFFFFFFull;
// Boards per lane and task at most: the split rule -- a spot of `boards` boards is cut into
// ceil(boards / (64 * lpt)) equal tasks of one wavefront each, so a spot of up to 64 * lpt boards is ONE task.
int eq_lpt(size_t m);

struct EqOut {            // any may be NULL
    uint32_t *win, *tie;
    uint64_t *share;
    uint32_t *boards;
    uint8_t *status;
};
struct EqSpots {          // the explicit form
    const uint8_t *holes, *board, *nboard;
    const uint16_t *live;
};
struct EqTables {         // the table form: a handle's own state (read only)
    const uint32_t *cards;
    const uint64_t *seat_states;
    const uint32_t *cursors;
    const int32_t *tables;   // NULL: spot i is table i
    int T;
};

// C(n, k), 0 <= k <= 5, n <= 52: exact at every step (r * (n - j) is a multiple of j + 1)
__host__ __device__ inline uint32_t eq_binom(uint32_t n, uint32_t k) {
    if (k > n) return 0;
    uint32_t r = 1;
    for (uint32_t j = 0; j < k; ++j) r = r * (n - j) / (j + 1);
    return r;
}

// ---- what the persistent enumeration kernels (k_equity<N>, k_ev<N>) share on the device
// The wavefront's pool: card j (canonical order) of the cards not dead, as its bit in the suit-lane layout; the empty slot holds none.
// The wavefront alone reads and writes mypool, between fences: the task before is done with it, the lanes see what the others wrote.
__device__ __forceinline__ void eq_fill_wave_pool(uint64_t *mypool, uint64_t avail, uint32_t lane) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (lane < 52u && ((avail >> lane) & 1ull))
        mypool[PK_IDX(__popcll(avail & ((1ull << lane) - 1ull)), 64, "mypool")] = card_bit(lane);
    if (lane == COMB_FROZEN) mypool[COMB_FROZEN] = 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Queues the whole call on `stream`: control block reset, descriptors + zeroed outputs + task list (one lane per spot), then the
// persistent enumeration kernel.  tab: the evaluator table (eval7_table); `tables` non-NULL selects the table form.
hipError_t eq_launch(hipStream_t stream, const uint32_t *tab, const EqSpots *spots, const EqTables *tables, int N, size_t m, const EqOut &out,
                     const EqWork &w, int lpt);

}  // namespace pk
