// pk_equity_ev.hpp -- showdown EV in chips: the side pots of Game.end_hand enumerated over every board (include/pokerl_hip.h "Showdown EV",
// DESIGN.md section 3.7): what the host entry points (pk_api.hip) and the kernels (pk_equity_ev.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pk_equity.hpp"

namespace pk {

// Levels a task compares per board (a task is spot x chunk of boards x GROUP of levels): the share counters of a group live in
// registers, EV_GROUP * N of them.  A spot at N seats has at most N - 1 levels to compare (the last stand is not compared).
__host__ __device__ constexpr int ev_group(int N) { return N <= 8 ? 3 : 2; }
__host__ __device__ constexpr int ev_groups_max(int N) { return (N - 1 + ev_group(N) - 1) / ev_group(N); }

// A level's record in the per-spot level table (u32 [m][N], index = the level's position in the visiting order):
//   bits 0-15 the remain mask, 16-23 the seat visited, 24 EXISTS, 25 LAST (the last stand: no comparison), 26 COMPARE (amount > 0, not LAST)
constexpr uint32_t EV_EXISTS = 1u << 24, EV_LAST = 1u << 25, EV_COMPARE = 1u << 26;

// Work space of one call, laid out by ev_layout: section 3.1's (control block, descriptors, task list -- a task's second word is
// chunk | group << 24), the level table, the bets as the kernels use them (the table form: bets + pending_bets), the amounts, and the share
// counters when the caller did not ask for them.
struct EvWork {
    EqWork eq;
    uint32_t *levels;     // [m][N]
    double *bets;         // [m][N]
    double *amount;       // [m][N]
    uint64_t *share;      // [m][N][N], NULL: the caller's array is used
};
size_t ev_layout(int N, size_t m, int lpt, int pool_max, bool own_share, char *base, EvWork *w);
size_t ev_task_cap(int N, size_t m, int lpt, int pool_max);

struct EvOut {            // any but status may be NULL
    uint64_t *share;      // [m][N][N] level-major
    uint8_t *level_seat;  // [m][N]
    double *amount;       // [m][N]
    double *ev;           // [m][N]
    uint32_t *boards;
    uint8_t *status;
};
struct EvTables {         // the table form: a handle's own state (read only)
    EqTables t;
    const double *bets, *pending;   // [N][T]
};

// Queues the whole call on `stream`: control block reset, k_ev_prep (checks, levels, zeroed counters, task list), the persistent enumeration
// kernel k_ev<N>, then k_ev_finish (one lane per spot and seat forms ev).  `tables` non-NULL selects the table form.
hipError_t ev_launch(hipStream_t stream, const uint32_t *tab, const EqSpots *spots, const double *bets, const EvTables *tables, int N, size_t m,
                     const EvOut &out, const EvWork &w, int lpt);

}  // namespace pk
