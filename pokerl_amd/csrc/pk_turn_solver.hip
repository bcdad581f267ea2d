// pk_turn_solver.hip -- the turn subgame solver (include/pokerl_hip.h "Turn solver"): simultaneous CFR+ for two
// players on a FOUR-card board, through the river card, in 64-bit integers whose sums do not depend on their order.  Two kernels:
//   k_ts_prep       one lane per spot: checks the four board cards and the dead mask, writes the spot's descriptor and its status;
//   k_turn_solve    k_river_solve's structure (pk_river_solver.hip) with a card loop around the river-level pass: a persistent grid of
//                   512-thread workgroups, ONE SPOT PER WORKGROUP at a time.  Once per spot and river card the holdings of the pool without
//                   that card are ranked on the five cards and sorted; what the card's passes need stays in the work space: per sorted
//                   position its turn slot and the bounds [lb, ub) of its key, per turn slot its position.  TURN-LEVEL arrays are indexed
//                   by the spot's fixed turn slot (the pair index of the holding's two pool slots), a lane owns slots tid, tid + 512,
//                   tid + 1024; RIVER-LEVEL arrays by the card's sorted position, a lane owns positions tid, tid + 512, tid + 1024.
//                   An iteration walks down the turn-level nodes, then for each river card -- one after the other, a barrier between
//                   them -- gathers the reaches at every chance node through the card's table, walks the river-level nodes down,
//                   evaluates their terminals as k_river_solve does (one 64-bit prefix sum for both players, card removal by the
//                   holder's own positions), walks up with the regret update fused in, and the owner of each position adds its root
//                   value into the chance node's value at its turn slot (positions map to distinct slots: no atomics); then it walks up
//                   the turn-level nodes.  A turn-level fold needs no order: the total minus the two per-card sums plus the own reach.
//                   Regrets and accumulators of river-level nodes are kept per card; values, reaches and probabilities of river-level
//                   nodes are rewritten by every card's pass.  The final passes run in the same launch.
//   k_trees_turn_solve   the same body (ts_solve_body<PER_SPOT>) for a call in which every spot names its tree: behind
//                   k_ts_prep comes k_trees_prep (pk_river_solver.hip); a spot stages trees[tree_of[spot]] (a refused one tree 0) into LDS at its top and lays
//                   the workgroup's slice -- sized for the call's largest nt and nr -- out for its own; `strategy` and `river_strategy`
//                   have the call's row strides, the rows at or past the spot's own counts are written 0.
//   k_lock_turn_solve   the same body with LOCK ("Locked nodes"): a locked turn-level node's probabilities stay in SG; a locked
//                   river-level node's are packed, per card and position, into the regret word of its first edge, which nothing else uses.
//   k_resolve_turn_solve   the same body with RESOLVE ("Re-solving"): the root's reaches come from the caller in the solver's
//                   own units, and the owners write both players' reaches, values and best-response values at the node the spot names: a
//                   turn-level node's after the last walk up, by turn slot; a river-level node's under the river card the spot names, inside
//                   the final pass's card loop after that card's walk up, by sorted position (the next card rewrites them).
//   k_resume_turn_solve   the same body with RESUME ("Resuming a solve"): the regrets and the average accumulators of both
//                   levels come from and go back to the caller's memory, before the final passes take the memory of R and A.
// Ordinary vector stores and LDS loads / stores only; no atomics, no scratch memory (tests/test_turn_solver_host.py reads the code object).
#include <hip/hip_runtime.h>

#include "pk_equity_common.hpp"
#include "pk_solver_common.hpp"
#include "pk_turn_solver.hpp"

using namespace pk;

#define TS_PREP_BLOCK 256

struct TsPrepArgs {
    TsSpots s;
    uint8_t *status;
    uint64_t *desc;
    size_t m;
};

__global__ void __launch_bounds__(TS_PREP_BLOCK) k_ts_prep(TsPrepArgs a) {
    const size_t i = (size_t)blockIdx.x * TS_PREP_BLOCK + threadIdx.x;
    if (i >= a.m) return;
    uint64_t *d = a.desc + i * (size_t)RS_DESC_WORDS;
    uint32_t status = 0;
    uint64_t dead = 0, known = 0;
    for (int j = 0; j < 4; ++j) {
        const uint32_t c = a.s.board[i * 4 + j];
        if (c >= 0x40u || (c & 15u) >= 13u) { status |= PK_EQ_BAD_CARD; continue; }
        const uint64_t bit = 1ull << ((c & 15u) * 4u + (c >> 4));              // canonical index (cards.py:77)
        status |= (dead & bit) ? (uint32_t)PK_EQ_DUP_CARD : 0u;
        dead |= bit;
        known |= 4ull << c;
    }
    const uint64_t out_of_play = a.s.dead ? a.s.dead[i] : 0ull;
    if (out_of_play >> 52) status |= PK_EQ_BAD_CARD;
    const uint64_t dd = out_of_play & 0x000FFFFFFFFFFFFFull;
    if (dd & dead) status |= PK_EQ_DUP_CARD;
    dead |= dd;
    const uint32_t P = 52u - (uint32_t)__popcll(dead);
    if (P < 5u) status |= PK_EQ_SMALL_POOL;                                    // two holdings that share no card, and a river card
    d[0] = known;
    d[1] = ~dead & 0x000FFFFFFFFFFFFFull;
    d[2] = (uint64_t)(status ? 0u : 1u) | ((uint64_t)P << 56);
    if (a.status) a.status[i] = (uint8_t)status;
}

namespace {

// the arrays of one level of the tree as a pass sees them: [node of the level][stride], cnt entries of a node in use
struct TsLevel {
    int64_t *R, *A, *U0, *U1;
    uint64_t *RR;
    uint32_t *SG;
    uint32_t stride, cnt;
};

}  // namespace

// The solver's body.  PER_SPOT = false: `tree` is the call's one tree (the kernel's argument), staged once per workgroup.  PER_SPOT = true:
// `tree` is the call's array of packed trees in device memory, and a spot stages trees[tree_of[spot]] (a refused one tree 0) -- after the barrier at the top
// of the spot, which the last use of `tr` by the spot before lies behind; ntmax, nrmax, Dtmax and Drmax are the call's largest.
// LOCK (with PER_SPOT; "Locked nodes"): a locked TURN-LEVEL node's probabilities are formed once per spot and stay in SG at its
// edges, as in the river solver.  A locked RIVER-LEVEL node's are formed once per spot and card and PACKED, four 16-bit fields, into the regret
// word of its first edge under that card -- a word no pass uses, since a locked node's regrets are never read or updated; every pass of the card unpacks
// them into SG, which the passes of the other cards rewrite.  The last pass of a card unpacks (the average stage) before the best responses take
// the memory of R and A.  A NULL tree_of: every spot uses tree 0.
// RESOLVE (with LOCK; "Re-solving"): rz.reach, where given, is the root's reaches; the node outputs of node rz.at[spot], which
// k_resolve_prep (pk_river_solver.hip) has seen below n, and for a river-level node rz.at_card[spot] in the pool.
// RESUME (with RESOLVE; "Resuming a solve"): rm.regret / rm.average (turn level, the layout of `strategy`) and rm.river_regret /
// rm.river_average (river level, the layout of `river_strategy`) are the caller's R and A, rm.t0[spot] the iterations they hold (NULL: 0).  A spot
// with t0 > 0 starts from them (clamped) at its free rows and runs t = t0 + 1 .. t0 + iters; after the last iteration and BEFORE the average-strategy
// stage -- the final passes take the memory of R and A -- the owners write both back, a turn-level entry by its turn slot, a river-level one by its
// sorted position under each card.  A locked river-level node's packed word never leaves: its row is skipped.  A spot with t0 = 0 reads nothing and
// has every other entry of its slices written 0; a refused spot's slices are not touched.
template <bool PER_SPOT, bool LOCK = false, bool RESOLVE = false, bool RESUME = false>
static __device__ __forceinline__ void ts_solve_body(const uint32_t *__restrict__ tab, const uint64_t *__restrict__ desc, const TsTree *tree, const TsTrees &mx,
                                                     const TsSpots &spots, const TsOut &out, char *ws, uint32_t iters, uint32_t m,
                                                     const TsLock &lk = TsLock{}, const TsResolve &rz = TsResolve{}, const TsResume &rm = TsResume{}) {
    static_assert(PER_SPOT || !LOCK, "the locked call has the tree-per-spot form only");
    static_assert(LOCK || !RESOLVE, "the re-solving call is the locked call with more arguments");
    static_assert(RESOLVE || !RESUME, "the resuming call is the re-solving call with more arguments");
    __shared__ uint32_t T[EVAL7_TAB_WORDS];
    __shared__ uint64_t slot[RS_SLOTS];               // key << 11 | turn slot, sorted once per spot and card; all ones = no holding.  Between
                                                      // the sorts the same memory holds rs and posof, or a turn-level fold's reaches
    __shared__ uint64_t pre[RS_PREFIX];               // pre[i]: both players' reach at sorted positions 0 .. i - 1; a turn-level fold: per-card sums
    __shared__ uint64_t pool[64];                     // card j of the pool (canonical order) as its bit in the suit-lane layout
    __shared__ uint32_t canon[64];                    // ... and its canonical index
    __shared__ uint64_t wsum[RS_WAVES];
    __shared__ TsTree tr;
    uint64_t *const rs = slot;                                                   // [RS_SORTED] a terminal's reaches in sorted order
    uint16_t *const posof = reinterpret_cast<uint16_t *>(slot + RS_SORTED);      // [TS_TURN] turn slot -> its sorted position under the card
    static_assert(RS_SORTED * 8 + TS_TURN * 2 <= RS_SLOTS * 8 && TS_TURN <= RS_SLOTS && RS_PREFIX >= 64, "rs and posof, or a fold's reaches, fit the sort slots");
    stage_eval7_tab<RS_BLOCK>(T, tab);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = uniform(tid >> 6);
    uint32_t n = 0, pot = 0, nt = 0, nr = 0, Dt = 0, Dr = 0;
    size_t rplane = 0;
    int64_t *Rt = nullptr, *At = nullptr, *U0t = nullptr, *U1t = nullptr, *Rr = nullptr, *Ar = nullptr, *U0r = nullptr, *U1r = nullptr;
    uint64_t *RRt = nullptr, *RRr = nullptr;
    uint32_t *SGt = nullptr, *SGr = nullptr, *bounds = nullptr;
    uint16_t *slotof = nullptr, *posofg = nullptr;
    TsLevel Lt{};
    // A tree into LDS (every lane of the workgroup comes here), and the workgroup's slice of the work space laid out for it
    auto stage = [&](const TsTree *src) {
        for (uint32_t w = tid; w < (uint32_t)(sizeof(TsTree) / 4); w += RS_BLOCK)
            reinterpret_cast<uint32_t *>(&tr)[PK_IDX(w, sizeof(TsTree) / 4, "tree")] = reinterpret_cast<const uint32_t *>(src)[w];
        __syncthreads();
        n = uniform(tr.n); pot = uniform(tr.pot); nt = uniform(tr.nt); nr = uniform(tr.nr);
        uint32_t dt = 0, dr = 0;
        for (uint32_t v = 0; v < n; ++v) {
            const bool dec = tr.kind[PK_IDX(v, TS_MAX_NODES, "kind")] <= RS_P1, riv = tr.river[PK_IDX(v, TS_MAX_NODES, "river")] != 0;
            dt += (dec && !riv) ? 1u : 0u;
            dr += (dec && riv) ? 1u : 0u;
        }
        Dt = uniform(dt); Dr = uniform(dr);
        // the workgroup's slice of the work space (pk_turn_solver.hpp): 64-bit arrays first
        char *const base = ws + (size_t)blockIdx.x * (PER_SPOT ? ts_group_bytes(mx.ntmax, mx.nrmax) : ts_group_bytes(nt, nr));
        const size_t tplane = (size_t)nt * TS_TURN;
        rplane = (size_t)nr * RS_SORTED;
        Rt = reinterpret_cast<int64_t *>(base); At = Rt + tplane; U0t = At + tplane; U1t = U0t + tplane;
        RRt = reinterpret_cast<uint64_t *>(U1t + tplane);
        Rr = reinterpret_cast<int64_t *>(RRt + tplane); Ar = Rr + rplane * TS_CARDS;                         // [card][river node][position]
        U0r = Ar + rplane * TS_CARDS; U1r = U0r + rplane;
        RRr = reinterpret_cast<uint64_t *>(U1r + rplane);
        SGt = reinterpret_cast<uint32_t *>(RRr + rplane); SGr = SGt + tplane;
        bounds = SGr + rplane;                                                   // [card][position] lb | ub << 16
        slotof = reinterpret_cast<uint16_t *>(bounds + (size_t)TS_CARDS * RS_SORTED);                          // [card][position] -> turn slot
        posofg = slotof + (size_t)TS_CARDS * RS_SORTED;                         // [card][turn slot] -> position
        Lt = TsLevel{Rt, At, U0t, U1t, RRt, SGt, (uint32_t)TS_TURN, 0u};
    };
    if constexpr (!PER_SPOT) stage(tree);
    auto idx = [&](uint32_t node) -> uint32_t { return uniform((uint32_t)tr.idx[PK_IDX(node, TS_MAX_NODES, "idx")]); };
    // where a node's entries begin in its level's arrays (wave-uniform: asked outside the code that depends on the lane), and entry i there
    auto row_of = [&](const TsLevel &L, uint32_t node) -> size_t { return (size_t)idx(node) * L.stride; };
    auto at = [&](const TsLevel &L, size_t row, uint32_t i) -> size_t { return row + PK_IDX(i, L.stride, "entry"); };
    auto tab_at = [&](uint32_t c, uint32_t i) -> size_t { return (size_t)PK_IDX(c, TS_CARDS, "card") * RS_SORTED + PK_IDX(i, RS_SORTED, "position"); };
    auto kids = [&](uint32_t node, uint32_t nact, uint32_t (&ch)[4]) {
#pragma unroll
        for (int a = 0; a < 4; ++a) ch[a] = (uint32_t)a < nact ? uniform((uint32_t)tr.child[PK_IDX(node, TS_MAX_NODES, "child")][a]) : 0u;
    };
    auto rows_of = [&](const TsLevel &L, const uint32_t (&ch)[4], uint32_t nact, size_t (&cr)[4]) {
#pragma unroll
        for (int a = 0; a < 4; ++a) cr[a] = (uint32_t)a < nact ? row_of(L, ch[a]) : 0;
    };
    auto kind_of = [&](uint32_t node) -> uint32_t { return uniform((uint32_t)tr.kind[PK_IDX(node, TS_MAX_NODES, "kind")]); };
    auto is_river = [&](uint32_t node) -> bool { return uniform((uint32_t)tr.river[PK_IDX(node, TS_MAX_NODES, "river")]) != 0u; };

    for (uint32_t spot = blockIdx.x; spot < m; spot += gridDim.x) {
        __syncthreads();                              // (the table and the tree; the spot before: its pool is done with)
        const uint64_t *d = desc + (size_t)spot * RS_DESC_WORDS;
        const uint64_t known = uniform(d[0]), meta = uniform(d[2]);
        const bool good = ((uint32_t)meta & 1u) != 0u;
        const uint64_t avail = good ? uniform(d[1]) : 0ull;     // (a refused spot: no holding is valid, every output is 0)
        const uint32_t P = (uint32_t)(meta >> 56);
        if constexpr (PER_SPOT) {
            // (good: k_trees_prep has seen tree_of[spot] < ntrees.  A refused spot stages tree 0, which always exists, and uses none of it:
            // staging on every path keeps the tree's counts and the slice's pointers plain values of the spot, not merges with the spot before)
            if constexpr (LOCK) stage(tree + ((good && mx.tree_of) ? PK_IDX(uniform(mx.tree_of[spot]), RS_MAX_TREES, "tree_of") : 0u));
            else stage(tree + (good ? PK_IDX(uniform(mx.tree_of[spot]), RS_MAX_TREES, "tree_of") : 0u));
            if (!good) { Dt = 0; Dr = 0; }
        }
        const uint32_t DtS = PER_SPOT ? mx.Dtmax : Dt, DrS = PER_SPOT ? mx.Drmax : Dr;               // the row strides of the strategies
        // ---- the iterations the spot's state holds; fresh: a solved spot that starts from nothing, whose unread state entries become 0
        uint32_t t0 = 0;
        bool fresh = false;
        if constexpr (RESUME) {
            t0 = (good && rm.t0) ? uniform(rm.t0[spot]) : 0u;
            fresh = good && t0 == 0u;
        }
        // ---- the node of the node outputs; a river-level one: the pool slot of its river card, whose holdings are no holdings there
        bool nodes = false, at_river = false;
        uint32_t an = 0, at_cs = 0;
        uint64_t at_avail = avail;
        if constexpr (RESOLVE) {
            nodes = rz.node_reach || rz.node_value || rz.node_br;
            if (nodes && good) {
                an = uniform((uint32_t)rz.at[spot]);
                at_river = is_river(an);
                if (at_river) {
                    const uint32_t c = uniform((uint32_t)rz.at_card[spot]), k = (c & 15u) * 4u + (c >> 4);
                    at_cs = (uint32_t)__popcll(avail & ((1ull << k) - 1ull));
                    at_avail = avail & ~(1ull << k);
                }
            }
        }
        // ---- zeros: every output at the holdings that are not in the pool, by the lanes of the fixed index h = tid + 512 j
        for (uint32_t h = tid; h < (uint32_t)RS_HOLDINGS; h += RS_BLOCK) {
            uint32_t ca = 0, cb = 1;
            unpair(h, ca, cb);
            if ((avail >> ca) & (avail >> cb) & 1ull) continue;
            for (uint32_t p = 0; p < 2u; ++p) {
                if (out.value) out.value[((size_t)spot * 2 + p) * RS_HOLDINGS + h] = 0;
                if (out.br) out.br[((size_t)spot * 2 + p) * RS_HOLDINGS + h] = 0;
            }
            if (out.strategy)
                for (uint32_t r = 0; r < DtS * 4u; ++r) out.strategy[((size_t)spot * DtS * 4 + r) * RS_HOLDINGS + h] = 0;
        }
        if constexpr (RESOLVE)
            if (nodes)
                for (uint32_t h = tid; h < (uint32_t)RS_HOLDINGS; h += RS_BLOCK) {
                    uint32_t ca = 0, cb = 1;
                    unpair(h, ca, cb);
                    if ((at_avail >> ca) & (at_avail >> cb) & 1ull) continue;
                    for (uint32_t p = 0; p < 2u; ++p) {
                        if (rz.node_reach) rz.node_reach[((size_t)spot * 2 + p) * RS_HOLDINGS + h] = 0;
                        if (rz.node_value) rz.node_value[((size_t)spot * 2 + p) * RS_HOLDINGS + h] = 0;
                        if (rz.node_br) rz.node_br[((size_t)spot * 2 + p) * RS_HOLDINGS + h] = 0;
                    }
                }
        // ... and of river_strategy every (card, holding) no pass writes: the card or the holding is not in the pool, or the holding has the card
        if (out.river_strategy)
            for (uint32_t e = tid; e < 52u * (uint32_t)RS_HOLDINGS; e += RS_BLOCK) {
                const uint32_t k = e / (uint32_t)RS_HOLDINGS, h = e - k * (uint32_t)RS_HOLDINGS;
                uint32_t ca = 0, cb = 1;
                unpair(h, ca, cb);
                if (((avail >> ca) & (avail >> cb) & (avail >> k) & 1ull) && k != ca && k != cb) continue;
                for (uint32_t r = 0; r < DrS; ++r)
                    for (uint32_t a = 0; a < 4u; ++a) out.river_strategy[((((size_t)spot * DrS + r) * 52 + k) * 4 + a) * RS_HOLDINGS + h] = 0;
            }
        // ... and, where the call's strides are wider than the spot's tree, the rows past its own at what the passes write
        if constexpr (PER_SPOT) {
            if (out.strategy && Dt < DtS)
                for (uint32_t h = tid; h < (uint32_t)RS_HOLDINGS; h += RS_BLOCK) {
                    uint32_t ca = 0, cb = 1;
                    unpair(h, ca, cb);
                    if (!((avail >> ca) & (avail >> cb) & 1ull)) continue;
                    for (uint32_t r = Dt * 4u; r < DtS * 4u; ++r) out.strategy[((size_t)spot * DtS * 4 + r) * RS_HOLDINGS + h] = 0;
                }
            if (out.river_strategy && Dr < DrS)
                for (uint32_t e = tid; e < 52u * (uint32_t)RS_HOLDINGS; e += RS_BLOCK) {
                    const uint32_t k = e / (uint32_t)RS_HOLDINGS, h = e - k * (uint32_t)RS_HOLDINGS;
                    uint32_t ca = 0, cb = 1;
                    unpair(h, ca, cb);
                    if (!(((avail >> ca) & (avail >> cb) & (avail >> k) & 1ull) && k != ca && k != cb)) continue;
                    for (uint32_t r = Dr; r < DrS; ++r)
                        for (uint32_t a = 0; a < 4u; ++a) out.river_strategy[((((size_t)spot * DrS + r) * 52 + k) * 4 + a) * RS_HOLDINGS + h] = 0;
                }
        }
        // ... and of a fresh spot's state every entry outside the pool's holdings (and cards) and every row past its own tree's
        if constexpr (RESUME)
            if (fresh) {
                for (uint32_t h = tid; h < (uint32_t)RS_HOLDINGS; h += RS_BLOCK) {
                    uint32_t ca = 0, cb = 1;
                    unpair(h, ca, cb);
                    const bool in = ((avail >> ca) & (avail >> cb) & 1ull) != 0ull;
                    for (uint32_t r = (in ? Dt : 0u) * 4u; r < DtS * 4u; ++r) {
                        rm.regret[((size_t)spot * DtS * 4 + r) * RS_HOLDINGS + h] = 0;
                        rm.average[((size_t)spot * DtS * 4 + r) * RS_HOLDINGS + h] = 0;
                    }
                }
                for (uint32_t e = tid; e < 52u * (uint32_t)RS_HOLDINGS; e += RS_BLOCK) {
                    const uint32_t k = e / (uint32_t)RS_HOLDINGS, h = e - k * (uint32_t)RS_HOLDINGS;
                    uint32_t ca = 0, cb = 1;
                    unpair(h, ca, cb);
                    const bool in = ((avail >> ca) & (avail >> cb) & (avail >> k) & 1ull) && k != ca && k != cb;
                    for (uint32_t r = in ? Dr : 0u; r < DrS; ++r)
                        for (uint32_t a = 0; a < 4u; ++a) {
                            rm.river_regret[((((size_t)spot * DrS + r) * 52 + k) * 4 + a) * RS_HOLDINGS + h] = 0;
                            rm.river_average[((((size_t)spot * DrS + r) * 52 + k) * 4 + a) * RS_HOLDINGS + h] = 0;
                        }
                }
            }
        if (!good) continue;
        fill_pool(pool, canon, avail, tid);
        const uint32_t nT = tri(P), nh = tri(P - 1u), K = P - 4u;
        uint32_t npad = 64;
        while (npad < nT) npad <<= 1;                 // (the P - 1 holdings with the card are all ones: a pad slot always exists)
        // ---- once per river card: rank, sort, and the card's tables
        for (uint32_t cs = 0; cs < P; ++cs) {
            __syncthreads();                          // (the pool; the card before: its slots have been read)
            for (uint32_t ph = tid; ph < npad; ph += RS_BLOCK) {
                uint64_t s = ~0ull;
                if (ph < nT) {
                    uint32_t ea, eb;
                    unpair(ph, ea, eb);
                    if (ea != cs && eb != cs) {
                        const uint64_t bits = known | pool[PK_IDX(cs, 64, "pool")] | pool[PK_IDX(ea, 64, "pool")] | pool[PK_IDX(eb, 64, "pool")];
                        s = ((uint64_t)order_key(eval7_tab_back(eval7_tab_front_bits(bits, T), T)) << 11) | ph;
                    }
                }
                slot[PK_IDX(ph, RS_SLOTS, "slot")] = s;
            }
            __syncthreads();
            for (uint32_t kk = 2; kk <= npad; kk <<= 1) {
                for (uint32_t jj = kk >> 1; jj > 0; jj >>= 1) {
                    for (uint32_t t = tid; t < (npad >> 1); t += RS_BLOCK) {
                        const uint32_t lo = ((t & ~(jj - 1u)) << 1) | (t & (jj - 1u)), hi = lo | jj;
                        const uint64_t a = slot[PK_IDX(lo, RS_SLOTS, "slot")], b = slot[PK_IDX(hi, RS_SLOTS, "slot")];
                        const bool up = (lo & kk) == 0u;
                        if ((a > b) == up) { slot[PK_IDX(lo, RS_SLOTS, "slot")] = b; slot[PK_IDX(hi, RS_SLOTS, "slot")] = a; }
                    }
                    __syncthreads();
                }
            }
#pragma unroll
            for (int j = 0; j < RS_PER_LANE; ++j) {
                const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                if (i >= nh) continue;
                const uint64_t s = slot[PK_IDX(i, RS_SLOTS, "slot")];
                const uint32_t kh = (uint32_t)(s >> 11), ph = (uint32_t)s & 2047u;
                uint32_t l = 0, u = 0;                                          // sorted positions with a key < kh, <= kh
                for (uint32_t step = npad >> 1; step > 0; step >>= 1) {
                    const uint32_t kl = (uint32_t)(slot[PK_IDX(l + step - 1u, RS_SLOTS, "slot")] >> 11);
                    const uint32_t ku = (uint32_t)(slot[PK_IDX(u + step - 1u, RS_SLOTS, "slot")] >> 11);
                    l += kl < kh ? step : 0u;
                    u += ku <= kh ? step : 0u;
                }
                slotof[tab_at(cs, i)] = (uint16_t)ph;
                bounds[tab_at(cs, i)] = l | (u << 16);
                posofg[(size_t)cs * TS_TURN + PK_IDX(ph, TS_TURN, "turn slot")] = (uint16_t)i;
            }
        }
        // ---- the turn slots this lane owns: their fixed indices
        uint32_t gh[RS_PER_LANE];
        auto fixed = [&](uint32_t s) -> uint32_t {
            uint32_t a, b;
            unpair(s, a, b);
            return tri(canon[PK_IDX(b, 64, "canon")]) + canon[PK_IDX(a, 64, "canon")];
        };
#pragma unroll
        for (int j = 0; j < RS_PER_LANE; ++j) {
            const uint32_t s = tid + (uint32_t)j * RS_BLOCK;
            gh[j] = s < nT ? fixed(s) : 0u;
        }
        auto river_level = [&](uint32_t cs) -> TsLevel {
            const size_t o = (size_t)PK_IDX(cs, TS_CARDS, "card") * rplane;
            return TsLevel{Rr + o, Ar + o, U0r, U1r, RRr, SGr, (uint32_t)RS_SORTED, nh};
        };
        TsLevel Lturn = Lt;
        Lturn.cnt = nT;
        // ---- the root's reaches; regrets and accumulators start at 0
        const uint16_t *w0 = spots.ranges + (size_t)spot * 2 * RS_HOLDINGS, *w1 = w0 + RS_HOLDINGS;
#pragma unroll
        for (int j = 0; j < RS_PER_LANE; ++j) {
            const uint32_t s = tid + (uint32_t)j * RS_BLOCK;
            if (s < nT) {
                bool from_ranges = true;
                if constexpr (RESOLVE)
                    if (rz.reach) {                   // (the solver's own units: no shift, the bound of a shifted weight)
                        const uint32_t *q = rz.reach + (size_t)spot * 2 * RS_HOLDINGS + PK_IDX(gh[j], RS_HOLDINGS, "reach");
                        const uint32_t q0 = q[0], q1 = q[RS_HOLDINGS];
                        RRt[at(Lturn, 0, s)] = (uint64_t)(q0 < TS_REACH_MAX ? q0 : TS_REACH_MAX) | ((uint64_t)(q1 < TS_REACH_MAX ? q1 : TS_REACH_MAX) << 32);
                        from_ranges = false;
                    }
                if (from_ranges)
                    RRt[at(Lturn, 0, s)] = ((uint64_t)w0[PK_IDX(gh[j], RS_HOLDINGS, "range")] << 1) | ((uint64_t)w1[PK_IDX(gh[j], RS_HOLDINGS, "range")] << 33);
                for (uint32_t v = 0; v < nt; ++v) { Rt[(size_t)v * TS_TURN + s] = 0; At[(size_t)v * TS_TURN + s] = 0; }
            }
            if (s < nh)
                for (uint32_t cs = 0; cs < P; ++cs)
                    for (uint32_t v = 0; v < nr; ++v) { Rr[((size_t)cs * nr + v) * RS_SORTED + s] = 0; Ar[((size_t)cs * nr + v) * RS_SORTED + s] = 0; }
        }
        // ---- the locked nodes of the spot (bit v of lockm[v >> 6]: decision node v), and their probabilities: the rule on the caller's weights
        uint64_t lockm[2] = {0, 0};
        auto locked_at = [&](uint32_t node) -> bool { return LOCK && ((lockm[(node >> 6) & 1u] >> (node & 63u)) & 1ull) != 0ull; };
        auto packed = [](const uint32_t (&sig)[4]) -> int64_t {
            return (int64_t)((uint64_t)sig[0] | ((uint64_t)sig[1] << 16) | ((uint64_t)sig[2] << 32) | ((uint64_t)sig[3] << 48));
        };
        if constexpr (LOCK) {
            for (uint32_t v = 0; v < n; ++v) {
                if (tr.kind[PK_IDX(v, TS_MAX_NODES, "kind")] > RS_P1) continue;
                const uint32_t row = tr.row[PK_IDX(v, TS_MAX_NODES, "row")];
                bool on = false;
                if (tr.river[PK_IDX(v, TS_MAX_NODES, "river")]) on = lk.river_lock && lk.river_lock[(size_t)spot * mx.Drmax + PK_IDX(row, mx.Drmax, "lock row")];
                else on = lk.lock && lk.lock[(size_t)spot * mx.Dtmax + PK_IDX(row, mx.Dtmax, "lock row")];
                lockm[v >> 6] |= on ? 1ull << (v & 63u) : 0ull;
            }
            lockm[0] = uniform(lockm[0]); lockm[1] = uniform(lockm[1]);
            for (uint32_t node = 0; node < n; ++node) {
                if (!locked_at(node)) continue;
                const uint32_t nact = uniform((uint32_t)tr.nact[PK_IDX(node, TS_MAX_NODES, "nact")]), row = uniform((uint32_t)tr.row[PK_IDX(node, TS_MAX_NODES, "row")]);
                uint32_t ch[4];
                kids(node, nact, ch);
                size_t cr[4];
                if (!is_river(node)) {
                    rows_of(Lturn, ch, nact, cr);
                    const uint16_t *src = lk.locked + ((size_t)spot * mx.Dtmax + row) * 4 * RS_HOLDINGS;
#pragma unroll
                    for (int j = 0; j < RS_PER_LANE; ++j) {
                        const uint32_t s = tid + (uint32_t)j * RS_BLOCK;
                        if (s >= nT) continue;
                        int64_t X[4];
                        uint32_t sig[4];
#pragma unroll
                        for (int a = 0; a < 4; ++a) X[a] = (uint32_t)a < nact ? (int64_t)src[(size_t)a * RS_HOLDINGS + PK_IDX(gh[j], RS_HOLDINGS, "locked")] : 0;
                        rs_sigma(X, nact, sig);
#pragma unroll
                        for (int a = 0; a < 4; ++a)
                            if ((uint32_t)a < nact) SGt[at(Lturn, cr[a], s)] = sig[a];
                    }
                    continue;
                }
                for (uint32_t cs = 0; cs < P; ++cs) {
                    const TsLevel L = river_level(cs);
                    rows_of(L, ch, nact, cr);
                    const uint16_t *src = lk.river_locked + (((size_t)spot * mx.Drmax + row) * 52 + canon[PK_IDX(cs, 64, "canon")]) * 4 * RS_HOLDINGS;
#pragma unroll
                    for (int j = 0; j < RS_PER_LANE; ++j) {
                        const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                        if (i >= nh) continue;
                        const uint32_t fx = fixed(slotof[tab_at(cs, i)]);
                        int64_t X[4];
                        uint32_t sig[4];
#pragma unroll
                        for (int a = 0; a < 4; ++a) X[a] = (uint32_t)a < nact ? (int64_t)src[(size_t)a * RS_HOLDINGS + PK_IDX(fx, RS_HOLDINGS, "river_locked")] : 0;
                        rs_sigma(X, nact, sig);
                        L.R[at(L, cr[0], i)] = packed(sig);
                    }
                }
            }
        }
        // ---- a resumed spot: R and A of its free rows from the caller's state, by the owner of each slot and of each card's positions.  The store
        // after the iterations is the same walk the other way: `load` false, and a fresh spot writes 0 at a locked row and past nact
        auto state_walk = [&](bool load) {
            for (uint32_t node = 0; node < n; ++node) {
                if (kind_of(node) > RS_P1) continue;
                const bool locked = locked_at(node);
                if (locked && (load || !fresh)) continue;
                const uint32_t nact = uniform((uint32_t)tr.nact[PK_IDX(node, TS_MAX_NODES, "nact")]), row = uniform((uint32_t)tr.row[PK_IDX(node, TS_MAX_NODES, "row")]);
                uint32_t ch[4];
                kids(node, nact, ch);
                size_t cr[4];
                if (!is_river(node)) {
                    rows_of(Lturn, ch, nact, cr);
                    const size_t o = ((size_t)spot * DtS + PK_IDX(row, DtS, "state row")) * 4 * RS_HOLDINGS;
#pragma unroll
                    for (int j = 0; j < RS_PER_LANE; ++j) {
                        const uint32_t s = tid + (uint32_t)j * RS_BLOCK;
                        if (s >= nT) continue;
#pragma unroll
                        for (int a = 0; a < 4; ++a) {
                            const bool live = (uint32_t)a < nact && !locked;
                            if (!(live || (fresh && !load))) continue;
                            const size_t g = o + (size_t)a * RS_HOLDINGS + PK_IDX(gh[j], RS_HOLDINGS, "state"), e = live ? at(Lturn, cr[a], s) : 0;
                            if (load) {
                                const int64_t r = rm.regret[g], v = rm.average[g];
                                Rt[e] = r < 0 ? 0 : r > TS_RESUME_RMAX ? TS_RESUME_RMAX : r;
                                At[e] = v < 0 ? 0 : v > TS_RESUME_AMAX ? TS_RESUME_AMAX : v;
                            } else {
                                rm.regret[g] = live ? Rt[e] : 0;
                                rm.average[g] = live ? At[e] : 0;
                            }
                        }
                    }
                    continue;
                }
                for (uint32_t cs = 0; cs < P; ++cs) {
                    const TsLevel L = river_level(cs);
                    rows_of(L, ch, nact, cr);
                    const size_t o = (((size_t)spot * DrS + PK_IDX(row, DrS, "state row")) * 52 + canon[PK_IDX(cs, 64, "canon")]) * 4 * RS_HOLDINGS;
#pragma unroll
                    for (int j = 0; j < RS_PER_LANE; ++j) {
                        const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                        if (i >= nh) continue;
                        const uint32_t fx = fixed(slotof[tab_at(cs, i)]);
#pragma unroll
                        for (int a = 0; a < 4; ++a) {
                            const bool live = (uint32_t)a < nact && !locked;
                            if (!(live || (fresh && !load))) continue;
                            const size_t g = o + (size_t)a * RS_HOLDINGS + PK_IDX(fx, RS_HOLDINGS, "state"), e = live ? at(L, cr[a], i) : 0;
                            if (load) {
                                const int64_t r = rm.river_regret[g], v = rm.river_average[g];
                                L.R[e] = r < 0 ? 0 : r > TS_RESUME_RMAX ? TS_RESUME_RMAX : r;
                                L.A[e] = v < 0 ? 0 : v > TS_RESUME_AMAX ? TS_RESUME_AMAX : v;
                            } else {
                                rm.river_regret[g] = live ? L.R[e] : 0;
                                rm.river_average[g] = live ? L.A[e] : 0;
                            }
                        }
                    }
                }
            }
        };
        if constexpr (RESUME)
            if (t0 > 0u) state_walk(true);
        auto unpack = [](int64_t w, uint32_t (&sig)[4]) {
#pragma unroll
            for (int a = 0; a < 4; ++a) sig[a] = (uint32_t)((uint64_t)w >> (16 * a)) & 0xFFFFu;
        };
        __syncthreads();                              // (the last card's slots have been read: their memory becomes rs and posof)

        // A river-level terminal under card cs (every lane of the workgroup comes here): k_river_solve's, the lane's positions from the tables
        auto terminal = [&](const TsLevel &L, uint32_t cs, uint32_t node, uint32_t kind) {
            const size_t nrow = row_of(L, node);
#pragma unroll
            for (int j = 0; j < RS_PER_LANE; ++j) {
                const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                if (i < nh) rs[PK_IDX(i, RS_SORTED, "rs")] = L.RR[at(L, nrow, i)];
            }
            __syncthreads();
            uint64_t v[RS_PER_LANE], mine = 0;
#pragma unroll
            for (int j = 0; j < RS_PER_LANE; ++j) {
                const uint32_t i = tid * RS_PER_LANE + (uint32_t)j;
                v[j] = i < nh ? rs[PK_IDX(i, RS_SORTED, "rs")] : 0ull;
                mine += v[j];
            }
            uint64_t inc = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint64_t y = __shfl_up(inc, off);
                inc += lane >= (uint32_t)off ? y : 0ull;
            }
            if (lane == 63u) wsum[PK_IDX(wave, RS_WAVES, "wsum")] = inc;
            __syncthreads();
            uint64_t run = inc - mine, all = 0;
#pragma unroll
            for (int w = 0; w < RS_WAVES; ++w) {
                const uint64_t s = wsum[PK_IDX(w, RS_WAVES, "wsum")];
                run += (uint32_t)w < wave ? s : 0ull;
                all += s;
            }
#pragma unroll
            for (int j = 0; j < RS_PER_LANE; ++j) {
                const uint32_t i = tid * RS_PER_LANE + (uint32_t)j;
                if (i < (uint32_t)RS_PREFIX) pre[PK_IDX(i, RS_PREFIX, "pre")] = run;
                run += v[j];
            }
            __syncthreads();
            const uint32_t f = kind - RS_FOLD0, pf = tr.put[PK_IDX(node, TS_MAX_NODES, "put")][f & 1u], c = tr.put[PK_IDX(node, TS_MAX_NODES, "put")][0];
#pragma unroll
            for (int j = 0; j < RS_PER_LANE; ++j) {
                const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                if (i >= nh) continue;
                const uint32_t hph = slotof[tab_at(cs, i)], lu = bounds[tab_at(cs, i)], lb = lu & 0xFFFFu, ub = lu >> 16;
                uint32_t ha, hb;
                unpair(hph, ha, hb);
                const uint64_t below0 = pre[PK_IDX(lb, RS_PREFIX, "pre")], self = rs[PK_IDX(i, RS_SORTED, "rs")];
                uint64_t below = below0, equal = pre[PK_IDX(ub, RS_PREFIX, "pre")] - below0 - self, conf = self;
                // card removal: every holding {ha, x}, {hb, x} without the river card, by its own sorted position
                const uint32_t ta = tri(ha), tb = tri(hb);
#pragma unroll 4
                for (uint32_t x = 0; x < P; ++x) {
                    const bool own = x == ha || x == hb || x == cs;
                    const uint32_t tx = tri(x);
                    const uint32_t i0 = own ? hph : pair(ha, ta, x, tx), i1 = own ? hph : pair(hb, tb, x, tx);
                    const uint32_t p0 = posof[PK_IDX(i0, TS_TURN, "posof")], p1 = posof[PK_IDX(i1, TS_TURN, "posof")];
                    const uint64_t r0 = own ? 0ull : rs[PK_IDX(p0, RS_SORTED, "rs")], r1 = own ? 0ull : rs[PK_IDX(p1, RS_SORTED, "rs")];
                    conf += r0 + r1;
                    below -= (p0 < lb ? r0 : 0ull) + (p1 < lb ? r1 : 0ull);
                    equal -= ((p0 >= lb && p0 < ub) ? r0 : 0ull) + ((p1 >= lb && p1 < ub) ? r1 : 0ull);
                }
                const uint64_t S = all - conf, above = S - below - equal;
                int64_t u0, u1;                       // player 0 meets player 1's reach (the high halves), player 1 the low ones
                if (kind == RS_SHOWDOWN) {
                    u0 = (int64_t)(2u * (pot + c)) * (int64_t)(below >> 32) + (int64_t)pot * (int64_t)(equal >> 32) - (int64_t)(2u * c) * (int64_t)(above >> 32);
                    u1 = (int64_t)(2u * (pot + c)) * (int64_t)(uint32_t)below + (int64_t)pot * (int64_t)(uint32_t)equal - (int64_t)(2u * c) * (int64_t)(uint32_t)above;
                } else {
                    const int64_t lose = -(int64_t)(2u * pf), gain = (int64_t)(2u * (pot + pf));
                    u0 = (f == 0u ? lose : gain) * (int64_t)(S >> 32);
                    u1 = (f == 1u ? lose : gain) * (int64_t)(uint32_t)S;
                }
                L.U0[at(L, nrow, i)] = u0;
                L.U1[at(L, nrow, i)] = u1;
            }
            __syncthreads();                          // (rs, pre and the totals are rewritten by the next terminal)
        };

        // A turn-level fold (every lane comes here): S_q(h) = the total - the sums of h's two cards + h's own entry, times the P - 4 river cards
        auto turn_fold = [&](uint32_t node, uint32_t kind) {
            const size_t nrow = row_of(Lturn, node);
#pragma unroll
            for (int j = 0; j < RS_PER_LANE; ++j) {
                const uint32_t s = tid + (uint32_t)j * RS_BLOCK;
                if (s < nT) slot[PK_IDX(s, RS_SLOTS, "slot")] = RRt[at(Lturn, nrow, s)];
            }
            __syncthreads();
            if (tid < P) {
                uint64_t sum = 0;
                const uint32_t tt = tri(tid);
                for (uint32_t x = 0; x < P; ++x) sum += x == tid ? 0ull : slot[PK_IDX(pair(tid, tt, x, tri(x)), RS_SLOTS, "slot")];
                pre[PK_IDX(tid, RS_PREFIX, "pre")] = sum;
            }
            __syncthreads();
            uint64_t twice = 0;
            for (uint32_t x = 0; x < P; ++x) twice += pre[PK_IDX(x, RS_PREFIX, "pre")];
            const uint64_t all = ((uint64_t)((uint32_t)twice >> 1)) | ((twice >> 33) << 32);       // (each half is even)
            const uint32_t f = kind - RS_FOLD0, pf = tr.put[PK_IDX(node, TS_MAX_NODES, "put")][f & 1u];
            const int64_t lose = -(int64_t)(2u * pf * K), gain = (int64_t)(2u * (pot + pf) * K);
#pragma unroll
            for (int j = 0; j < RS_PER_LANE; ++j) {
                const uint32_t s = tid + (uint32_t)j * RS_BLOCK;
                if (s >= nT) continue;
                uint32_t a, b;
                unpair(s, a, b);
                const uint64_t S = all - pre[PK_IDX(a, RS_PREFIX, "pre")] - pre[PK_IDX(b, RS_PREFIX, "pre")] + slot[PK_IDX(s, RS_SLOTS, "slot")];
                U0t[at(Lturn, nrow, s)] = (f == 0u ? lose : gain) * (int64_t)(S >> 32);
                U1t[at(Lturn, nrow, s)] = (f == 1u ? lose : gain) * (int64_t)(uint32_t)S;
            }
            __syncthreads();
        };

        // A decision node on the way down, at either level.  FROM_R: the probabilities come from the regrets and are kept in SG;
        // otherwise SG is played as it stands.
        auto decide_down = [&](const TsLevel &L, uint32_t node, uint32_t kind, bool walk_from_r) {
            const uint32_t nact = uniform((uint32_t)tr.nact[PK_IDX(node, TS_MAX_NODES, "nact")]);
            // (a locked node: SG holds what is played -- at the river level once the card's packed word has been unpacked into it)
            const bool from_r = walk_from_r && !locked_at(node), from_word = LOCK && walk_from_r && locked_at(node) && is_river(node);
            uint32_t ch[4];
            kids(node, nact, ch);
            size_t cr[4];
            rows_of(L, ch, nact, cr);
            const size_t nrow = row_of(L, node);
#pragma unroll
            for (int j = 0; j < RS_PER_LANE; ++j) {
                const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                if (i >= L.cnt) continue;
                uint32_t sig[4];
                if (from_r) {
                    int64_t X[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) X[a] = (uint32_t)a < nact ? L.R[at(L, cr[a], i)] : 0;
                    rs_sigma(X, nact, sig);
                }
                if constexpr (LOCK)
                    if (from_word) unpack(L.R[at(L, cr[0], i)], sig);
                const uint64_t rr = L.RR[at(L, nrow, i)];
                const uint32_t r0 = (uint32_t)rr, r1 = (uint32_t)(rr >> 32);
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    if ((uint32_t)a >= nact) continue;
                    const size_t e = at(L, cr[a], i);
                    if (from_r || from_word) L.SG[e] = sig[a]; else sig[a] = L.SG[e];
                    const uint32_t mine = (uint32_t)(((uint64_t)(kind == RS_P0 ? r0 : r1) * sig[a]) >> 15);
                    L.RR[e] = kind == RS_P0 ? ((uint64_t)mine | ((uint64_t)r1 << 32)) : ((uint64_t)r0 | ((uint64_t)mine << 32));
                }
            }
        };
        // ... and on the way up of iteration t, with the regret and accumulator updates
        auto decide_up = [&](const TsLevel &L, uint32_t node, uint32_t kind, uint32_t t) {
            const uint32_t nact = uniform((uint32_t)tr.nact[PK_IDX(node, TS_MAX_NODES, "nact")]);
            int64_t *const Up = kind == RS_P0 ? L.U0 : L.U1, *const Uq = kind == RS_P0 ? L.U1 : L.U0;
            uint32_t ch[4];
            kids(node, nact, ch);
            size_t cr[4];
            rows_of(L, ch, nact, cr);
            const size_t nrow = row_of(L, node);
#pragma unroll
            for (int j = 0; j < RS_PER_LANE; ++j) {
                const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                if (i >= L.cnt) continue;
                int64_t up[4], acc = 0, uq = 0;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    up[a] = 0;
                    if ((uint32_t)a >= nact) continue;
                    const size_t e = at(L, cr[a], i);
                    up[a] = Up[e];
                    acc += (int64_t)L.SG[e] * up[a];
                    uq += Uq[e];
                }
                const int64_t un = acc >> 15;         // (the sum first, the floor once)
                Up[at(L, nrow, i)] = un;
                Uq[at(L, nrow, i)] = uq;
                if (locked_at(node)) continue;        // (neither R nor A is updated at a locked node)
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    if ((uint32_t)a >= nact) continue;
                    const size_t e = at(L, cr[a], i);
                    const int64_t r = L.R[e] + up[a] - un;
                    L.R[e] = r > 0 ? r : 0;
                    const uint64_t rr = L.RR[e];
                    L.A[e] += (int64_t)((uint64_t)t * (uint64_t)(kind == RS_P0 ? (uint32_t)rr : (uint32_t)(rr >> 32)));
                }
            }
        };
        // ... of the last pass: beside each player's value, the value of the player who plays the maximum at its own nodes (B0 / B1, in
        // the memory of R / A; a terminal's is its value)
        auto decide_up_best = [&](const TsLevel &L, uint32_t node, uint32_t kind) {
            const uint32_t nact = uniform((uint32_t)tr.nact[PK_IDX(node, TS_MAX_NODES, "nact")]);
            int64_t *const Up = kind == RS_P0 ? L.U0 : L.U1, *const Uq = kind == RS_P0 ? L.U1 : L.U0;
            int64_t *const Bp = kind == RS_P0 ? L.R : L.A, *const Bq = kind == RS_P0 ? L.A : L.R;
            uint32_t ch[4];
            bool leaf[4];
            kids(node, nact, ch);
            size_t cr[4];
            rows_of(L, ch, nact, cr);
            const size_t nrow = row_of(L, node);
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const uint32_t k = kind_of(ch[a]);
                leaf[a] = k > RS_P1 && k != (uint32_t)TS_CHANCE;
            }
#pragma unroll
            for (int j = 0; j < RS_PER_LANE; ++j) {
                const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                if (i >= L.cnt) continue;
                int64_t acc = 0, uq = 0, bp = 0, bq = 0;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    if ((uint32_t)a >= nact) continue;
                    const size_t e = at(L, cr[a], i);
                    const int64_t up = Up[e], uqa = Uq[e], bpa = leaf[a] ? up : Bp[e], bqa = leaf[a] ? uqa : Bq[e];
                    acc += (int64_t)L.SG[e] * up;
                    uq += uqa;
                    bp = (a == 0 || bpa > bp) ? bpa : bp;
                    bq += bqa;
                }
                Up[at(L, nrow, i)] = acc >> 15;
                Uq[at(L, nrow, i)] = uq;
                Bp[at(L, nrow, i)] = bp;
                Bq[at(L, nrow, i)] = bq;
            }
        };
        // The turn-level walk down: reaches, the folds' values; a chance node's sums start at 0 (BEST: those of the best responses too)
        auto turn_down = [&](bool from_r, bool best) {
            for (uint32_t node = 0; node < n; ++node) {
                if (is_river(node)) continue;
                const uint32_t kind = kind_of(node);
                if (kind <= RS_P1) { decide_down(Lturn, node, kind, from_r); continue; }
                if (kind != (uint32_t)TS_CHANCE) { turn_fold(node, kind); continue; }
                const size_t nrow = row_of(Lturn, node);
#pragma unroll
                for (int j = 0; j < RS_PER_LANE; ++j) {
                    const uint32_t s = tid + (uint32_t)j * RS_BLOCK;
                    if (s >= nT) continue;
                    U0t[at(Lturn, nrow, s)] = 0; U1t[at(Lturn, nrow, s)] = 0;
                    if (best) { Rt[at(Lturn, nrow, s)] = 0; At[at(Lturn, nrow, s)] = 0; }
                }
            }
        };
        // A card's pass begins: its positions into LDS (the barrier also orders the card before: its sums into the chance nodes)
        auto card_begin = [&](uint32_t cs) {
            for (uint32_t s = tid; s < nT; s += RS_BLOCK) posof[PK_IDX(s, TS_TURN, "posof")] = posofg[(size_t)cs * TS_TURN + s];
            __syncthreads();
        };
        // The river-level walk down under card cs: a chance node hands its reaches to its child through the card's table
        auto river_down = [&](const TsLevel &L, uint32_t cs, bool from_r) {
            for (uint32_t node = 0; node < n; ++node) {
                const uint32_t kind = kind_of(node);
                if (kind == (uint32_t)TS_CHANCE) {
                    const uint32_t ch = uniform((uint32_t)tr.child[PK_IDX(node, TS_MAX_NODES, "child")][0]);
                    const size_t nrow = row_of(Lturn, node), crow = row_of(L, ch);
#pragma unroll
                    for (int j = 0; j < RS_PER_LANE; ++j) {
                        const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                        if (i < nh) L.RR[at(L, crow, i)] = RRt[at(Lturn, nrow, slotof[tab_at(cs, i)])];
                    }
                    continue;
                }
                if (!is_river(node)) continue;
                if (kind <= RS_P1) decide_down(L, node, kind, from_r);
                else terminal(L, cs, node, kind);
            }
        };

        // ---- the iterations
        for (uint32_t t = 1; t <= iters; ++t) {
            const uint32_t tw = RESUME ? t0 + t : t;  // (the iteration's number: all that t enters is the accumulators' weight)
            turn_down(true, false);
            for (uint32_t cs = 0; cs < P; ++cs) {
                const TsLevel L = river_level(cs);
                card_begin(cs);
                river_down(L, cs, true);
                for (uint32_t node = n; node-- > 0u;) {
                    const uint32_t kind = kind_of(node);
                    if (kind == (uint32_t)TS_CHANCE) {
                        const uint32_t ch = uniform((uint32_t)tr.child[PK_IDX(node, TS_MAX_NODES, "child")][0]);
                        const size_t nrow = row_of(Lturn, node), crow = row_of(L, ch);
#pragma unroll
                        for (int j = 0; j < RS_PER_LANE; ++j) {
                            const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                            if (i >= nh) continue;
                            const size_t e = at(Lturn, nrow, slotof[tab_at(cs, i)]);
                            U0t[e] += L.U0[at(L, crow, i)];
                            U1t[e] += L.U1[at(L, crow, i)];
                        }
                    } else if (is_river(node) && kind <= RS_P1) decide_up(L, node, kind, tw);
                }
            }
            __syncthreads();                          // (the last card's sums)
            for (uint32_t node = n; node-- > 0u;) {
                const uint32_t kind = kind_of(node);
                if (!is_river(node) && kind <= RS_P1) decide_up(Lturn, node, kind, tw);
            }
        }
        // ---- the state goes back to the caller, before the final passes take the memory of R and A
        if constexpr (RESUME) state_walk(false);

        // ---- the average strategy: the rule applied to the accumulators; it stays in SG for the last walk
        auto average = [&](const TsLevel &L, uint32_t node, uint32_t cs, bool river) {
            const uint32_t nact = uniform((uint32_t)tr.nact[PK_IDX(node, TS_MAX_NODES, "nact")]), row = uniform((uint32_t)tr.row[PK_IDX(node, TS_MAX_NODES, "row")]);
            uint32_t ch[4];
            kids(node, nact, ch);
            size_t cr[4];
            rows_of(L, ch, nact, cr);
            const size_t nrow = row_of(L, node);
#pragma unroll
            for (int j = 0; j < RS_PER_LANE; ++j) {
                const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                if (i >= L.cnt) continue;
                int64_t X[4];
                uint32_t sig[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) X[a] = (uint32_t)a < nact ? L.A[at(L, cr[a], i)] : 0;
                if (locked_at(node)) {
                    if (river) unpack(L.R[at(L, cr[0], i)], sig);
                    else {
#pragma unroll
                        for (int a = 0; a < 4; ++a) sig[a] = (uint32_t)a < nact ? L.SG[at(L, cr[a], i)] : 0u;
                    }
                } else rs_sigma(X, nact, sig);
                uint16_t *o = nullptr;
                if (river) {
                    if (out.river_strategy)
                        o = out.river_strategy + ((((size_t)spot * DrS + row) * 52 + canon[PK_IDX(cs, 64, "canon")]) * 4) * RS_HOLDINGS + fixed(slotof[tab_at(cs, i)]);
                } else if (out.strategy) o = out.strategy + (((size_t)spot * DtS + row) * 4) * RS_HOLDINGS + gh[j];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    if ((uint32_t)a < nact) L.SG[at(L, cr[a], i)] = sig[a];
                    if (o) o[(size_t)a * RS_HOLDINGS] = (uint16_t)sig[a];
                }
            }
        };
        for (uint32_t node = 0; node < n; ++node)
            if (!is_river(node) && kind_of(node) <= RS_P1) average(Lturn, node, 0u, false);
        const bool values = out.value || out.br || nodes;
        if (!(values || out.river_strategy)) continue;
        // ---- its values and the best responses against it: one walk down serves all three, the walk up carries the maximum beside the value
        if (values) turn_down(false, true);
        for (uint32_t cs = 0; cs < P; ++cs) {
            const TsLevel L = river_level(cs);
            for (uint32_t node = 0; node < n; ++node)
                if (is_river(node) && kind_of(node) <= RS_P1) average(L, node, cs, true);
            if (!values) continue;
            card_begin(cs);
            river_down(L, cs, false);
            for (uint32_t node = n; node-- > 0u;) {
                const uint32_t kind = kind_of(node);
                if (kind == (uint32_t)TS_CHANCE) {
                    const uint32_t ch = uniform((uint32_t)tr.child[PK_IDX(node, TS_MAX_NODES, "child")][0]);
                    const size_t nrow = row_of(Lturn, node), crow = row_of(L, ch);
                    const bool leaf = kind_of(ch) > RS_P1;
#pragma unroll
                    for (int j = 0; j < RS_PER_LANE; ++j) {
                        const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                        if (i >= nh) continue;
                        const size_t e = at(Lturn, nrow, slotof[tab_at(cs, i)]), g = at(L, crow, i);
                        const int64_t u0 = L.U0[g], u1 = L.U1[g];
                        U0t[e] += u0;
                        U1t[e] += u1;
                        Rt[e] += leaf ? u0 : L.R[g];
                        At[e] += leaf ? u1 : L.A[g];
                    }
                } else if (is_river(node) && kind <= RS_P1) decide_up_best(L, node, kind);
            }
            if constexpr (RESOLVE)
                if (at_river && cs == at_cs) {        // the node's outputs under this card: the next card rewrites what they are read from
                    const uint32_t k = kind_of(an);
                    const bool leaf = k > RS_P1;
                    const size_t nrow = row_of(L, an);
#pragma unroll
                    for (int j = 0; j < RS_PER_LANE; ++j) {
                        const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                        if (i >= nh) continue;
                        const size_t o = (size_t)spot * 2 * RS_HOLDINGS + PK_IDX(fixed(slotof[tab_at(cs, i)]), RS_HOLDINGS, "holding"), e = at(L, nrow, i);
                        if (rz.node_reach) { const uint64_t rr = L.RR[e]; rz.node_reach[o] = (uint32_t)rr; rz.node_reach[o + RS_HOLDINGS] = (uint32_t)(rr >> 32); }
                        if (rz.node_value) { rz.node_value[o] = L.U0[e]; rz.node_value[o + RS_HOLDINGS] = L.U1[e]; }
                        if (rz.node_br) { rz.node_br[o] = leaf ? L.U0[e] : L.R[e]; rz.node_br[o + RS_HOLDINGS] = leaf ? L.U1[e] : L.A[e]; }
                    }
                }
        }
        if (!values) continue;
        __syncthreads();                              // (the last card's sums)
        for (uint32_t node = n; node-- > 0u;) {
            const uint32_t kind = kind_of(node);
            if (!is_river(node) && kind <= RS_P1) decide_up_best(Lturn, node, kind);
        }
#pragma unroll
        for (int j = 0; j < RS_PER_LANE; ++j) {
            const uint32_t s = tid + (uint32_t)j * RS_BLOCK;
            if (s >= nT) continue;
            const size_t o = (size_t)spot * 2 * RS_HOLDINGS + gh[j];
            if (out.value) { out.value[o] = U0t[at(Lturn, 0, s)]; out.value[o + RS_HOLDINGS] = U1t[at(Lturn, 0, s)]; }
            if (out.br) { out.br[o] = Rt[at(Lturn, 0, s)]; out.br[o + RS_HOLDINGS] = At[at(Lturn, 0, s)]; }
        }
        if constexpr (RESOLVE)
            if (nodes && !at_river) {
                const uint32_t k = kind_of(an);
                const bool leaf = k > RS_P1 && k != (uint32_t)TS_CHANCE;       // (a fold's best response is its value; a chance node carries its sums)
                const size_t nrow = row_of(Lturn, an);
#pragma unroll
                for (int j = 0; j < RS_PER_LANE; ++j) {
                    const uint32_t s = tid + (uint32_t)j * RS_BLOCK;
                    if (s >= nT) continue;
                    const size_t o = (size_t)spot * 2 * RS_HOLDINGS + gh[j], e = at(Lturn, nrow, s);
                    if (rz.node_reach) { const uint64_t rr = RRt[e]; rz.node_reach[o] = (uint32_t)rr; rz.node_reach[o + RS_HOLDINGS] = (uint32_t)(rr >> 32); }
                    if (rz.node_value) { rz.node_value[o] = U0t[e]; rz.node_value[o + RS_HOLDINGS] = U1t[e]; }
                    if (rz.node_br) { rz.node_br[o] = leaf ? U0t[e] : Rt[e]; rz.node_br[o + RS_HOLDINGS] = leaf ? U1t[e] : At[e]; }
                }
            }
    }
}

// registers: one workgroup per CU is two waves per SIMD
__global__ void __launch_bounds__(RS_BLOCK, 2) k_turn_solve(const uint32_t *__restrict__ tab, const uint64_t *__restrict__ desc, TsTree tree, TsSpots spots,
                                                            TsOut out, char *ws, uint32_t iters, uint32_t m) {
    ts_solve_body<false>(tab, desc, &tree, TsTrees{}, spots, out, ws, iters, m);
}
__global__ void __launch_bounds__(RS_BLOCK, 2) k_trees_turn_solve(const uint32_t *__restrict__ tab, const uint64_t *__restrict__ desc, TsTrees trees, TsSpots spots,
                                                                  TsOut out, char *ws, uint32_t iters, uint32_t m) {
    ts_solve_body<true>(tab, desc, trees.trees, trees, spots, out, ws, iters, m);
}

// the locked call: k_trees_turn_solve's body with LOCK (the name does not begin with k_turn_solve or k_trees_: host tests list those)
__global__ void __launch_bounds__(RS_BLOCK, 2) k_lock_turn_solve(const uint32_t *__restrict__ tab, const uint64_t *__restrict__ desc, TsTrees trees, TsLock lk,
                                                                 TsSpots spots, TsOut out, char *ws, uint32_t iters, uint32_t m) {
    ts_solve_body<true, true>(tab, desc, trees.trees, trees, spots, out, ws, iters, m, lk);
}

// the re-solving call: k_lock_turn_solve's body with RESOLVE (the name begins with none of the prefixes host tests list kernels by)
__global__ void __launch_bounds__(RS_BLOCK, 2) k_resolve_turn_solve(const uint32_t *__restrict__ tab, const uint64_t *__restrict__ desc, TsTrees trees, TsLock lk,
                                                                    TsResolve rz, TsSpots spots, TsOut out, char *ws, uint32_t iters, uint32_t m) {
    ts_solve_body<true, true, true>(tab, desc, trees.trees, trees, spots, out, ws, iters, m, lk, rz);
}

// the resuming call: k_resolve_turn_solve's body with RESUME (the name begins with none of the prefixes host tests list kernels by)
__global__ void __launch_bounds__(RS_BLOCK, 2) k_resume_turn_solve(const uint32_t *__restrict__ tab, const uint64_t *__restrict__ desc, TsTrees trees, TsLock lk,
                                                                   TsResolve rz, TsResume rm, TsSpots spots, TsOut out, char *ws, uint32_t iters, uint32_t m) {
    ts_solve_body<true, true, true, true>(tab, desc, trees.trees, trees, spots, out, ws, iters, m, lk, rz, rm);
}

namespace pk {

hipError_t ts_launch(hipStream_t stream, const uint32_t *tab, const TsSpots &spots, const TsTree &tree, uint32_t iters, size_t m, const TsOut &out,
                     char *work) {
    if (m == 0) return hipSuccess;
    const TsPrepArgs a{spots, out.status, (uint64_t *)work, m};
    hipLaunchKernelGGL(k_ts_prep, dim3((unsigned)((m + TS_PREP_BLOCK - 1) / TS_PREP_BLOCK)), dim3(TS_PREP_BLOCK), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !(out.strategy || out.river_strategy || out.value || out.br)) return e;   // (status alone: the preparation kernel has written it)
    hipLaunchKernelGGL(k_turn_solve, dim3(ts_grid(m, tree.nt, tree.nr)), dim3(RS_BLOCK), 0, stream, tab, (const uint64_t *)work, tree, spots, out,
                       work + rs_desc_bytes(m), iters, (uint32_t)m);
    return hipGetLastError();
}

hipError_t ts_launch_trees(hipStream_t stream, const uint32_t *tab, const TsSpots &spots, const TsTrees &trees, uint32_t ntrees, uint32_t iters, size_t m,
                           const TsOut &out, char *work) {
    if (m == 0) return hipSuccess;
    const TsPrepArgs a{spots, out.status, (uint64_t *)work, m};
    hipLaunchKernelGGL(k_ts_prep, dim3((unsigned)((m + TS_PREP_BLOCK - 1) / TS_PREP_BLOCK)), dim3(TS_PREP_BLOCK), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = trees_prep_launch(stream, trees.tree_of, ntrees, (uint64_t *)work, out.status, m);
    if (e != hipSuccess || !(out.strategy || out.river_strategy || out.value || out.br)) return e;   // (status alone: the preparation kernels have written it)
    hipLaunchKernelGGL(k_trees_turn_solve, dim3(ts_grid(m, trees.ntmax, trees.nrmax)), dim3(RS_BLOCK), 0, stream, tab, (const uint64_t *)work, trees, spots,
                       out, work + rs_desc_bytes(m), iters, (uint32_t)m);
    return hipGetLastError();
}

hipError_t ts_launch_locked(hipStream_t stream, const uint32_t *tab, const TsSpots &spots, const TsTrees &trees, uint32_t ntrees, const TsLock &lk,
                            uint32_t iters, size_t m, const TsOut &out, char *work) {
    if (m == 0) return hipSuccess;
    const TsPrepArgs a{spots, out.status, (uint64_t *)work, m};
    hipLaunchKernelGGL(k_ts_prep, dim3((unsigned)((m + TS_PREP_BLOCK - 1) / TS_PREP_BLOCK)), dim3(TS_PREP_BLOCK), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && trees.tree_of) e = trees_prep_launch(stream, trees.tree_of, ntrees, (uint64_t *)work, out.status, m);
    if (e != hipSuccess || !(out.strategy || out.river_strategy || out.value || out.br)) return e;   // (status alone: the preparation kernels have written it)
    hipLaunchKernelGGL(k_lock_turn_solve, dim3(ts_grid(m, trees.ntmax, trees.nrmax)), dim3(RS_BLOCK), 0, stream, tab, (const uint64_t *)work, trees, lk, spots,
                       out, work + rs_desc_bytes(m), iters, (uint32_t)m);
    return hipGetLastError();
}

hipError_t ts_launch_resolve(hipStream_t stream, const uint32_t *tab, const TsSpots &spots, const TsTrees &trees, uint32_t ntrees, const TsLock &lk,
                             const TsResolve &rz, uint32_t iters, size_t m, const TsOut &out, char *work) {
    if (m == 0) return hipSuccess;
    const TsPrepArgs a{spots, out.status, (uint64_t *)work, m};
    hipLaunchKernelGGL(k_ts_prep, dim3((unsigned)((m + TS_PREP_BLOCK - 1) / TS_PREP_BLOCK)), dim3(TS_PREP_BLOCK), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && trees.tree_of) e = trees_prep_launch(stream, trees.tree_of, ntrees, (uint64_t *)work, out.status, m);
    if (e == hipSuccess && rz.at)
        e = resolve_prep_launch(stream, trees.trees, (uint32_t)sizeof(TsTree), (uint32_t)offsetof(TsTree, river), trees.tree_of, rz.at, rz.at_card, (uint64_t *)work,
                                out.status, m);
    if (e != hipSuccess || !(out.strategy || out.river_strategy || out.value || out.br || rz.at)) return e;   // (status alone: the preparation kernels have written it)
    hipLaunchKernelGGL(k_resolve_turn_solve, dim3(ts_grid(m, trees.ntmax, trees.nrmax)), dim3(RS_BLOCK), 0, stream, tab, (const uint64_t *)work, trees, lk, rz,
                       spots, out, work + rs_desc_bytes(m), iters, (uint32_t)m);
    return hipGetLastError();
}

hipError_t ts_launch_resume(hipStream_t stream, const uint32_t *tab, const TsSpots &spots, const TsTrees &trees, uint32_t ntrees, const TsLock &lk,
                            const TsResolve &rz, const TsResume &rm, uint32_t iters, size_t m, const TsOut &out, char *work) {
    if (m == 0) return hipSuccess;
    const TsPrepArgs a{spots, out.status, (uint64_t *)work, m};
    hipLaunchKernelGGL(k_ts_prep, dim3((unsigned)((m + TS_PREP_BLOCK - 1) / TS_PREP_BLOCK)), dim3(TS_PREP_BLOCK), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && trees.tree_of) e = trees_prep_launch(stream, trees.tree_of, ntrees, (uint64_t *)work, out.status, m);
    if (e == hipSuccess && rz.at)
        e = resolve_prep_launch(stream, trees.trees, (uint32_t)sizeof(TsTree), (uint32_t)offsetof(TsTree, river), trees.tree_of, rz.at, rz.at_card, (uint64_t *)work,
                                out.status, m);
    if (e == hipSuccess && rm.t0) e = resume_prep_launch(stream, rm.t0, iters, (uint64_t *)work, out.status, m);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_resume_turn_solve, dim3(ts_grid(m, trees.ntmax, trees.nrmax)), dim3(RS_BLOCK), 0, stream, tab, (const uint64_t *)work, trees, lk, rz, rm,
                       spots, out, work + rs_desc_bytes(m), iters, (uint32_t)m);
    return hipGetLastError();
}

}  // namespace pk
