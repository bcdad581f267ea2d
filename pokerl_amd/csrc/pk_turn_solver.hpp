// pk_turn_solver.hpp -- the turn subgame solver: heads-up CFR+ on a four-card board through the river card, one subgame per workgroup, in
// integers (include/pokerl_hip.h "Turn solver"): what the host entry points (pk_api.hip) and the kernels
// (pk_turn_solver.hip) share.  The table kernels do not include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pk_river_solver.hpp"

namespace pk {

constexpr int TS_MAX_NODES = PK_TS_MAX_NODES;
constexpr int TS_CARDS = 48;                             // river cards of the largest pool
constexpr int TS_TURN_HOLDINGS = 1128;                   // C(48, 2): holdings of the largest pool on a four-card board
constexpr int TS_TURN = 1152;                            // ... padded: slots per turn-level node (NOT RS_SORTED: 1088 < 1128)
constexpr size_t TS_WORK_MAX = (size_t)4 << 30;          // the ceiling of the per-workgroup slices together (not measured: DESIGN.md 3.13)
static_assert(RS_BLOCK * RS_PER_LANE >= TS_TURN_HOLDINGS && TS_TURN >= TS_TURN_HOLDINGS && TS_TURN % 64 == 0 && TS_TURN_HOLDINGS < 2048, "a lane owns at most RS_PER_LANE slots");

enum { TS_CHANCE = 5 };

// The tree as the kernel takes it (by value).  Derived by the host check: nact, row (a decision node's row of `strategy` or of
// `river_strategy`), river (1 below a chance node) and idx (the node's number among the nodes of its level: where its arrays are).
struct TsTree {
    uint32_t n, pot, nt, nr;                             // nodes, chips in the middle, turn-level and river-level nodes (nt + nr = n)
    uint32_t put[TS_MAX_NODES][2];
    uint8_t kind[TS_MAX_NODES], nact[TS_MAX_NODES], row[TS_MAX_NODES], river[TS_MAX_NODES], idx[TS_MAX_NODES];
    uint8_t child[TS_MAX_NODES][4];
};
static_assert(sizeof(TsTree) % 4 == 0 && sizeof(TsTree) <= 3072, "copied into LDS as 32-bit words; travels as a kernel argument (4 KB with the rest)");

struct TsSpots {
    const uint8_t *board;      // [m][4]
    const uint64_t *dead;      // [m], NULL: none
    const uint16_t *ranges;    // [m][2][1326]
};
struct TsOut {                 // any may be NULL
    uint16_t *strategy;        // [m][D_t][4][1326]
    uint16_t *river_strategy;  // [m][D_r][52][4][1326]
    int64_t *value, *br;       // [m][2][1326]
    uint8_t *status;           // [m]
};

// Work space: the m descriptors, then -- sized by the grid, never by m, and for the largest pool -- per workgroup:
//   the 48 river cards' tables: per sorted position its turn slot (u16) and the bounds of its key (u16, u16), per turn slot its position (u16);
//   per turn-level node and slot: regret, accumulator, both values, both reaches (one word), the edge's probability;
//   per river-level node, card and position: regret and accumulator -- all that outlives a card's pass;
//   per river-level node and position: both values, both reaches, the probability -- rewritten by every card's pass.
constexpr size_t TS_TABLE_BYTES = (size_t)TS_CARDS * (RS_SORTED * 6 + TS_TURN * 2);
constexpr size_t TS_TURN_NODE_BYTES = (size_t)TS_TURN * (5 * 8 + 4);
constexpr size_t TS_RIVER_NODE_BYTES = (size_t)RS_SORTED * ((size_t)TS_CARDS * 16 + 3 * 8 + 4);
constexpr size_t ts_group_bytes(uint32_t nt, uint32_t nr) { return TS_TABLE_BYTES + nt * TS_TURN_NODE_BYTES + nr * TS_RIVER_NODE_BYTES; }
constexpr unsigned ts_grid(size_t m, uint32_t nt, uint32_t nr) {
    const size_t fit = TS_WORK_MAX / ts_group_bytes(nt, nr), cap = fit < (size_t)RS_GRID_MAX ? fit : (size_t)RS_GRID_MAX;
    return (unsigned)(m < cap ? m : cap);
}
constexpr size_t ts_work_bytes(size_t m, uint32_t nt, uint32_t nr, bool solve) {
    return rs_desc_bytes(m) + (solve ? (size_t)ts_grid(m, nt, nr) * ts_group_bytes(nt, nr) : 0);
}
static_assert(ts_group_bytes(1, TS_MAX_NODES - 1) * 16 < TS_WORK_MAX, "the largest tree still gets a grid");

// Queues the whole call on `stream`: descriptors + status (one lane per spot), then -- where an output beside status is wanted -- the
// persistent kernel.  tab: the evaluator table (eval7_table).  The tree has passed the host check (pk_api.hip ts_check_tree).
hipError_t ts_launch(hipStream_t stream, const uint32_t *tab, const TsSpots &spots, const TsTree &tree, uint32_t iters, size_t m, const TsOut &out,
                     char *work);

// ---- a tree per spot (include/pokerl_hip.h "River and turn solvers: a tree per spot")
struct TsTrees {
    const TsTree *trees;               // [ntrees] packed trees, DEVICE memory
    const uint32_t *tree_of;           // [m], device memory
    uint32_t ntmax, nrmax;             // the largest nt and nr over the call's trees: a workgroup's slice and the grid
    uint32_t Dtmax, Drmax;             // the largest D_t and D_r: the row strides of `strategy` and `river_strategy`
};
constexpr size_t ts_trees_bytes(uint32_t ntrees) { return ((size_t)ntrees * sizeof(TsTree) + 255) & ~(size_t)255; }
// ts_launch's launches with k_trees_prep between them and k_trees_turn_solve; `work` as ts_work_bytes(m, trees.ntmax, trees.nrmax, solve) sizes it.
hipError_t ts_launch_trees(hipStream_t stream, const uint32_t *tab, const TsSpots &spots, const TsTrees &trees, uint32_t ntrees, uint32_t iters, size_t m,
                           const TsOut &out, char *work);

// ---- locked nodes (include/pokerl_hip.h "Locked nodes")
struct TsLock {
    const uint8_t *lock;            // [m][Dtmax], nonzero: the turn-level row is locked; NULL: none is
    const uint16_t *locked;         // [m][Dtmax][4][1326], the layout of `strategy`
    const uint8_t *river_lock;      // [m][Drmax], a river-level row, for all river cards at once; NULL: none is
    const uint16_t *river_locked;   // [m][Drmax][52][4][1326], the layout of `river_strategy`
};
// ts_launch_trees's launches with k_lock_turn_solve; trees.tree_of may be NULL (every spot uses tree 0: k_trees_prep is not queued).
hipError_t ts_launch_locked(hipStream_t stream, const uint32_t *tab, const TsSpots &spots, const TsTrees &trees, uint32_t ntrees, const TsLock &lk,
                            uint32_t iters, size_t m, const TsOut &out, char *work);


// ---- re-solving (include/pokerl_hip.h "Re-solving"): root reaches in the solver's own units, and both players' reaches,
// values and best-response values at one node of the spot's tree -- of a river-level node under river card at_card.  Any member may be NULL.
constexpr uint32_t TS_REACH_MAX = (1u << 17) - 1u;       // a root reach: what a u16 weight << 1 never exceeds
struct TsResolve {
    const uint32_t *reach;     // [m][2][1326]; non-NULL: the root reaches, `ranges` is not read
    const uint8_t *at;         // [m] the node of the node outputs; NULL exactly when all three are
    const uint8_t *at_card;    // [m] a card code, read for a river-level at
    uint32_t *node_reach;      // [m][2][1326]
    int64_t *node_value, *node_br;
};
// ts_launch_locked's launches with k_resolve_prep (pk_river_solver.hip; where rz.at is given) and k_resolve_turn_solve
hipError_t ts_launch_resolve(hipStream_t stream, const uint32_t *tab, const TsSpots &spots, const TsTrees &trees, uint32_t ntrees, const TsLock &lk,
                             const TsResolve &rz, uint32_t iters, size_t m, const TsOut &out, char *work);


// ---- resuming (include/pokerl_hip.h "Resuming a solve"): the regrets and the average accumulators of both levels, IN and
// OUT in the caller's memory, and the number of iterations they hold.  The four arrays are given together (the host check); t0 may be NULL (all 0).
constexpr int64_t TS_RESUME_RMAX = ((int64_t)1 << 60) - 1;   // what a loaded regret / accumulator is clamped to: the header's bounds for 4 096
constexpr int64_t TS_RESUME_AMAX = ((int64_t)1 << 41) - 1;   // iterations, so that 4 096 further ones still fit (its arithmetic is there)
struct TsResume {
    const uint32_t *t0;                    // [m]
    int64_t *regret, *average;             // [m][Dtmax][4][1326], the layout of `strategy`
    int64_t *river_regret, *river_average; // [m][Drmax][52][4][1326], the layout of `river_strategy`
};
// ts_launch_resolve's launches with k_resume_prep (pk_river_solver.hip; where rm.t0 is given) and k_resume_turn_solve; the four state arrays are
// not NULL.  The solve kernel always runs: the state is an output
hipError_t ts_launch_resume(hipStream_t stream, const uint32_t *tab, const TsSpots &spots, const TsTrees &trees, uint32_t ntrees, const TsLock &lk,
                            const TsResolve &rz, const TsResume &rm, uint32_t iters, size_t m, const TsOut &out, char *work);

}  // namespace pk
