// pk_preflop_solver.hpp -- the pre-flop solver: heads-up CFR+ over a caller's betting tree with no board, a showdown paid by the resident
// matchup table (include/pokerl_hip.h "Pre-flop solver"): what the host entry points (pk_api.hip) and the kernel
// (pk_preflop_solver.hip) share.  The trees, the outputs and the packed form are the river solver's (pk_river_solver.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pk_preflop.hpp"
#include "pk_river_solver.hpp"

namespace pk {

constexpr int PS_BLOCK = RS_BLOCK, PS_WAVES = PS_BLOCK / 64;
constexpr int PS_PER_LANE = 3;                           // holdings a lane owns: h = tid, tid + 512, tid + 1024
constexpr int PS_GRID_MAX = 256;                         // persistent grid: one 512-thread workgroup per CU at most
constexpr uint32_t PS_BOARDS = PK_PREFLOP_BOARDS;           // B = C(48, 5): the boards of one matchup, win + tie + lose of a disjoint pair
constexpr int PS_STRIDE = 1344;                          // 1326 holdings padded to whole wavefronts: a node's row of every work-space array
static_assert(PS_BLOCK * PS_PER_LANE >= RS_HOLDINGS && PS_STRIDE >= RS_HOLDINGS && PS_STRIDE % 64 == 0, "a lane owns at most PS_PER_LANE holdings");
static_assert(PFM_HOLDINGS == RS_HOLDINGS, "the matchup table and the ranges share the holding index");

// Work space -- sized by the grid, never by m -- per workgroup and per (node, holding): the regret and the average accumulator of the edge
// INTO the node, both players' values, both players' reaches (one 64-bit word) and the edge's probability.
constexpr size_t PS_NODE_BYTES = (size_t)PS_STRIDE * (5 * 8 + 4);
constexpr unsigned ps_grid(size_t m) { return (unsigned)(m < (size_t)PS_GRID_MAX ? m : (size_t)PS_GRID_MAX); }
constexpr size_t ps_group_bytes(uint32_t n) { return (size_t)n * PS_NODE_BYTES; }
constexpr size_t ps_work_bytes(size_t m, uint32_t nmax, bool solve) { return solve ? (size_t)ps_grid(m) * ps_group_bytes(nmax) : 0; }

// Queues the call on `stream`: ONE launch, which also writes `status` (there is no preparation kernel: a spot has no cards to check).
// M: the resident matchup table (win, then tie).  trees.trees: ntrees packed trees that have passed the host check, device memory;
// trees.tree_of: device memory, or NULL (every spot uses tree 0).  work: ps_work_bytes(m, trees.nmax, strategy || value || br).
hipError_t ps_launch(hipStream_t stream, const uint32_t *M, const uint16_t *ranges, const RsTrees &trees, uint32_t ntrees, uint32_t iters, size_t m,
                     const RsOut &out, char *work);

}  // namespace pk
