// pk_river_solver.hpp -- the river subgame solver: heads-up CFR+ over a caller's betting tree, one subgame per workgroup, in integers
// (include/pokerl_hip.h "River solver"): what the host entry points (pk_api.hip) and the kernels
// (pk_river_solver.hip) share.  The table kernels do not include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pk_equity.hpp"

namespace pk {

constexpr int RS_HOLDINGS = PK_EQ_HOLDINGS;              // C(52, 2): the fixed holding index of the ranges and of every output
constexpr int RS_BLOCK = 512, RS_WAVES = RS_BLOCK / 64;
constexpr int RS_PER_LANE = 3;                           // sorted positions a lane owns: i = tid, tid + 512, tid + 1024
constexpr int RS_GRID_MAX = 256;                         // persistent grid: one 512-thread workgroup per CU (its work space is megabytes)
constexpr int RS_MAX_NODES = PK_RS_MAX_NODES, RS_MAX_ITERS = PK_RS_MAX_ITERS;
constexpr uint32_t RS_MAX_CHIPS = PK_RS_MAX_CHIPS;
constexpr uint32_t RS_ONE = PK_RS_ONE;                   // a probability of 1 (Q15)
constexpr int RS_POOL_HOLDINGS = 1081;                   // C(47, 2): holdings of the largest pool (five board cards are always gone)
constexpr int RS_SORTED = 1088;                          // ... padded: sorted positions per node of the work space and of the LDS arrays
constexpr int RS_PREFIX = RS_SORTED + 8;                 // exclusive prefix sums: positions 0 .. nh inclusive
constexpr int RS_SLOTS = 2048;                           // sort slots: the next power of two
constexpr int RS_DESC_WORDS = 3;                         // a spot's descriptor: as range vs range's (pk_equity_rvr.hpp), k = 0
static_assert(RS_BLOCK * RS_PER_LANE >= RS_POOL_HOLDINGS && RS_SORTED >= RS_POOL_HOLDINGS && RS_SORTED % 8 == 0, "a lane owns at most RS_PER_LANE positions");

enum { RS_P0 = 0, RS_P1 = 1, RS_FOLD0 = 2, RS_FOLD1 = 3, RS_SHOWDOWN = 4 };
enum { RS_GIVEN = 6 };                                   // a terminal whose values the caller supplies ("Re-solving"; 5 is the turn solver's chance node)

// The tree as the kernel takes it (by value: it travels with the launch, so the caller's host arrays are done with when the call returns).
// nact and row are derived by the host check: a decision node's number of children, and its row of `strategy`.
struct RsTree {
    uint32_t n, pot;
    uint32_t put[RS_MAX_NODES][2];
    uint8_t kind[RS_MAX_NODES], nact[RS_MAX_NODES], row[RS_MAX_NODES];
    uint8_t child[RS_MAX_NODES][4];
};
static_assert(sizeof(RsTree) % 4 == 0 && sizeof(RsTree) <= 1024, "copied into LDS as 32-bit words");

struct RsSpots {
    const uint8_t *board;      // [m][5]
    const uint64_t *dead;      // [m], NULL: none
    const uint16_t *ranges;    // [m][2][1326]
};
struct RsOut {                 // any may be NULL
    uint16_t *strategy;        // [m][D][4][1326]
    int64_t *value, *br;       // [m][2][1326]
    uint8_t *status;           // [m]
};

// Work space: the m descriptors, then -- sized by the grid, never by m -- per workgroup and per (node, sorted position): the regret and the
// average accumulator of the edge INTO the node, both players' values, both players' reaches (one 64-bit word) and the edge's probability.
constexpr size_t RS_NODE_BYTES = (size_t)RS_SORTED * (5 * 8 + 4);
constexpr unsigned rs_grid(size_t m) { return (unsigned)(m < (size_t)RS_GRID_MAX ? m : (size_t)RS_GRID_MAX); }
constexpr size_t rs_desc_bytes(size_t m) { return (m * RS_DESC_WORDS * sizeof(uint64_t) + 255) & ~(size_t)255; }
constexpr size_t rs_group_bytes(uint32_t n) { return (size_t)n * RS_NODE_BYTES; }
constexpr size_t rs_work_bytes(size_t m, uint32_t n, bool solve) { return rs_desc_bytes(m) + (solve ? (size_t)rs_grid(m) * rs_group_bytes(n) : 0); }

// Queues the whole call on `stream`: descriptors + status (one lane per spot), then -- where strategy, value or br is wanted -- the
// persistent kernel.  tab: the evaluator table (eval7_table).  The tree has passed the host check (pk_api.hip rs_check_tree).
hipError_t rs_launch(hipStream_t stream, const uint32_t *tab, const RsSpots &spots, const RsTree &tree, uint32_t iters, size_t m, const RsOut &out,
                     char *work);

// ---- a tree per spot (include/pokerl_hip.h "River and turn solvers: a tree per spot")
constexpr uint32_t RS_MAX_TREES = PK_RS_MAX_TREES;
struct RsTrees {
    const RsTree *trees;       // [ntrees] packed trees, DEVICE memory
    const uint32_t *tree_of;   // [m], device memory
    uint32_t nmax, Dmax;       // the largest n and D over the call's trees: a workgroup's slice, the row stride of `strategy`
};
constexpr size_t rs_trees_bytes(uint32_t ntrees) { return ((size_t)ntrees * sizeof(RsTree) + 255) & ~(size_t)255; }
// k_trees_prep on the m descriptors k_rs_prep or k_ts_prep has written (the turn solver's launch calls it too)
hipError_t trees_prep_launch(hipStream_t stream, const uint32_t *tree_of, uint32_t ntrees, uint64_t *desc, uint8_t *status, size_t m);
// rs_launch's launches with k_trees_prep between them and k_trees_river_solve; `work` as rs_work_bytes(m, trees.nmax, solve) sizes it.
hipError_t rs_launch_trees(hipStream_t stream, const uint32_t *tab, const RsSpots &spots, const RsTrees &trees, uint32_t ntrees, uint32_t iters, size_t m,
                           const RsOut &out, char *work);


// ---- locked nodes (include/pokerl_hip.h "Locked nodes")
struct RsLock {
    const uint8_t *lock;       // [m][Dmax], nonzero: the row is locked; NULL: nothing is
    const uint16_t *locked;    // [m][Dmax][4][1326], the layout of `strategy`
};
// rs_launch_trees's launches with k_lock_river_solve; trees.tree_of may be NULL (every spot uses tree 0: k_trees_prep is not queued).
hipError_t rs_launch_locked(hipStream_t stream, const uint32_t *tab, const RsSpots &spots, const RsTrees &trees, uint32_t ntrees, const RsLock &lk,
                            uint32_t iters, size_t m, const RsOut &out, char *work);


// ---- re-solving (include/pokerl_hip.h "Re-solving"): root reaches in the solver's own units, a terminal of given values,
// and both players' reaches, values and best-response values at one node of the spot's tree.  Any member may be NULL.
constexpr uint32_t RS_REACH_MAX = (1u << 20) - 1u;       // a root reach: what a u16 weight << 4 never exceeds
constexpr int64_t RS_GIVEN_MAX = ((int64_t)1 << 45) - 1; // |a given value|: the bound every other terminal's value obeys
struct RsResolve {
    const uint32_t *reach;     // [m][2][1326]; non-NULL: the root reaches, `ranges` is not read
    const int64_t *given;      // [m][2][1326] the values at the spot's RS_GIVEN node
    const uint8_t *at;         // [m] the node of the node outputs; NULL exactly when all three are
    uint32_t *node_reach;      // [m][2][1326]
    int64_t *node_value, *node_br;
};
// k_resolve_prep, queued behind the other preparation kernels: one lane per spot that is still good.  at[i] >= the n of the spot's tree:
// PK_EQ_BAD_TREE; river_off != 0 (the turn solver: the byte offset of TsTree::river) and a river-level at[i] whose at_card[i] is no card of
// the pool: PK_EQ_BAD_CARD.  Either clears the descriptor's "good" bit.  trees: the packed trees, `stride` bytes each, n their first word.
hipError_t resolve_prep_launch(hipStream_t stream, const void *trees, uint32_t stride, uint32_t river_off, const uint32_t *tree_of, const uint8_t *at,
                               const uint8_t *at_card, uint64_t *desc, uint8_t *status, size_t m);
// rs_launch_locked's launches with k_resolve_prep (where rz.at is given) and k_resolve_river_solve
hipError_t rs_launch_resolve(hipStream_t stream, const uint32_t *tab, const RsSpots &spots, const RsTrees &trees, uint32_t ntrees, const RsLock &lk,
                             const RsResolve &rz, uint32_t iters, size_t m, const RsOut &out, char *work);


// ---- resuming (include/pokerl_hip.h "Resuming a solve"): the regrets and the average accumulators of a solve, IN and OUT
// in the caller's memory, and the number of iterations they hold.  regret and average are given together (the host check); t0 may be NULL (all 0).
constexpr int64_t RS_RESUME_RMAX = ((int64_t)1 << 58) - 1;   // what a loaded regret / accumulator is clamped to: the header's bounds for 4 096
constexpr int64_t RS_RESUME_AMAX = ((int64_t)1 << 44) - 1;   // iterations, so that 4 096 further ones still fit (its arithmetic is there)
struct RsResume {
    const uint32_t *t0;        // [m]
    int64_t *regret, *average; // [m][Dmax][4][1326], the layout of `strategy`
};
// k_resume_prep, queued behind the other preparation kernels: one lane per spot that is still good; t0[i] + iters > 4 096: PK_EQ_BAD_ITER,
// which clears the descriptor's "good" bit (the turn solver's launch calls it too)
hipError_t resume_prep_launch(hipStream_t stream, const uint32_t *t0, uint32_t iters, uint64_t *desc, uint8_t *status, size_t m);
// rs_launch_resolve's launches with k_resume_prep (where rm.t0 is given) and k_resume_river_solve; rm.regret and rm.average are not NULL.  The
// solve kernel always runs: the state is an output
hipError_t rs_launch_resume(hipStream_t stream, const uint32_t *tab, const RsSpots &spots, const RsTrees &trees, uint32_t ntrees, const RsLock &lk,
                            const RsResolve &rz, const RsResume &rm, uint32_t iters, size_t m, const RsOut &out, char *work);

}  // namespace pk
