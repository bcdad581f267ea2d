// pk_river_solver.hip -- the river subgame solver (include/pokerl_hip.h "River solver"): simultaneous CFR+ for two
// players over a caller's betting tree, in 64-bit integers whose sums do not depend on their order.  Two kernels, each in two forms:
//   k_rs_prep       one lane per spot: checks the five board cards and the dead mask, writes the spot's descriptor (range vs range's, k = 0)
//                   and its status;
//   k_river_solve   a persistent grid of 512-thread workgroups, the evaluator table and the tree in LDS (staged once per workgroup), ONE
//                   SPOT PER WORKGROUP at a time.  Per spot the pool's holdings are ranked and sorted ONCE (k_rvr's rank and order stage at
//                   k = 0); from then on a lane OWNS the holdings at sorted positions i = tid, tid + 512, tid + 1024: their regrets,
//                   average accumulators, reaches, probabilities and values, all in the workgroup's slice of the global work space, every
//                   word of which is read and written by its owner alone.  Only a terminal node couples lanes: both players' reaches
//                   go to LDS in sorted order as ONE 64-bit word (player 0 low, player 1 high: neither half of any sum reaches 2^31),
//                   a workgroup prefix sum follows, and a lane reads the weight below, equal to and above each of its holdings at the
//                   bounds it found once per spot; the 2 (P - 2) holdings that share a card with it, and itself, are taken back out by their
//                   own sorted positions (card removal by the holder's keys, as k_rvr's combine).
//                   The final passes (the average strategy, its values, the best responses) run in the same launch.  A best-response
//                   pass of p needs only q's reaches, which are those of the value pass: one walk down serves all three, and the walk up
//                   carries the maximum beside the value.
//   k_trees_prep / k_trees_river_solve   a call in which every spot names its tree ("River and turn solvers: a tree per spot", DESIGN.md
//                   section 3.14).  k_trees_prep follows k_rs_prep: it refuses a spot whose tree_of is >= ntrees (PK_EQ_BAD_TREE, folded into
//                   the descriptor's "good" bit).  k_trees_river_solve is k_river_solve's body (rs_solve_body<PER_SPOT>): it stages
//                   trees[tree_of[spot]] into LDS at the top of each spot (a refused one: tree 0, unused), lays its slice -- sized for the call's largest tree -- out
//                   for that tree's n, and writes `strategy` with the call's row stride Dmax, the rows at or past the spot's own D as zeros.
//   k_lock_river_solve   the same body with LOCK ("Locked nodes"): rows of the strategy fixed by the caller.  A locked node's
//                   probabilities are formed once per spot from the caller's weights and stay in SG; R and A are left alone there.
//   k_resolve_prep / k_resolve_river_solve   the same body with RESOLVE ("Re-solving"): the root's reaches come from the
//                   caller in the solver's own units, a terminal of kind RS_GIVEN takes its values from the caller, and the owners write both
//                   players' reaches, values and best-response values at the node the spot names.  k_resolve_prep follows the other
//                   preparation kernels and refuses a spot whose node (or, in the turn solver, river card) does not exist.
//   k_resume_prep / k_resume_river_solve   the same body with RESUME ("Resuming a solve"): the regrets and the average
//                   accumulators come from and go back to the caller's memory, a spot runs iterations t0 + 1 .. t0 + iters.  k_resume_prep refuses a
//                   spot whose t0 + iters passes 4 096 (PK_EQ_BAD_ITER); a refused spot's state is not touched.
// Ordinary vector stores and LDS loads / stores only; no atomics, no scratch memory (tests/test_river_solver_host.py reads the code object).
#include <hip/hip_runtime.h>

#include "pk_equity_common.hpp"
#include "pk_river_solver.hpp"
#include "pk_solver_common.hpp"

using namespace pk;

#define RS_PREP_BLOCK 256

struct RsPrepArgs {
    RsSpots s;
    uint8_t *status;
    uint64_t *desc;
    size_t m;
};

__global__ void __launch_bounds__(RS_PREP_BLOCK) k_rs_prep(RsPrepArgs a) {
    const size_t i = (size_t)blockIdx.x * RS_PREP_BLOCK + threadIdx.x;
    if (i >= a.m) return;
    uint64_t *d = a.desc + i * (size_t)RS_DESC_WORDS;
    uint32_t status = 0;
    uint64_t dead = 0, known = 0;
    for (int j = 0; j < 5; ++j) {
        const uint32_t c = a.s.board[i * 5 + j];
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
    if (P < 4u) status |= PK_EQ_SMALL_POOL;                                    // TWO holdings that share no card
    d[0] = known;
    d[1] = ~dead & 0x000FFFFFFFFFFFFFull;
    d[2] = (uint64_t)(status ? 0u : 1u) | ((uint64_t)P << 56);
    if (a.status) a.status[i] = (uint8_t)status;
}

// The second half of a tree-per-spot call's preparation, queued behind k_rs_prep or k_ts_prep (whose text and code stay as they are): one
// lane per spot, a tree_of >= ntrees adds PK_EQ_BAD_TREE to the spot's status and clears its descriptor's "good" bit, so that the solver
// never indexes the trees with it.
__global__ void __launch_bounds__(RS_PREP_BLOCK) k_trees_prep(const uint32_t *__restrict__ tree_of, uint32_t ntrees, uint64_t *desc, uint8_t *status, size_t m) {
    const size_t i = (size_t)blockIdx.x * RS_PREP_BLOCK + threadIdx.x;
    if (i >= m || tree_of[i] < ntrees) return;
    desc[i * (size_t)RS_DESC_WORDS + 2] &= ~1ull;
    if (status) status[i] |= (uint8_t)PK_EQ_BAD_TREE;
}

// The solver's body.  PER_SPOT = false: `tree` is the call's one tree (the kernel's argument), staged once per workgroup.  PER_SPOT = true:
// `tree` is the call's array of packed trees in device memory, and a spot stages trees[tree_of[spot]] (a refused one tree 0) -- after the barrier at the top
// of the spot, which the last use of `tr` by the spot before lies behind; nmax and Dmax are the largest n and D of the call.
// LOCK (with PER_SPOT; "Locked nodes"): rows of `lk.lock` fix a decision node's probabilities to the strategy rule applied to
// `lk.locked`.  They are formed once per spot by the owner of each position and stay in SG at the node's edges: the walk down plays SG as it stands
// there, the walk up leaves R and A alone, the average-strategy stage writes `strategy` from SG.  A NULL tree_of: every spot uses tree 0.
// RESOLVE (with LOCK; "Re-solving"): rz.reach, where given, is the root's reaches; an RS_GIVEN terminal's values are rz.given's;
// after the final walk up the owners write rz.node_reach / node_value / node_br at node rz.at[spot], which k_resolve_prep has seen below n.
// RESUME (with RESOLVE; "Resuming a solve"): rm.regret / rm.average are the caller's R and A in the layout of `strategy`,
// rm.t0[spot] the iterations they already hold (NULL: 0).  A spot with t0 > 0 starts from them (clamped) at its free rows and runs t = t0 + 1 ..
// t0 + iters; after the last iteration and BEFORE the average-strategy stage -- the final passes take the memory of R and A -- the owners write both
// back.  A spot with t0 = 0 reads nothing and has every other entry of its slice written 0; a refused spot's slice is not touched.
template <bool PER_SPOT, bool LOCK = false, bool RESOLVE = false, bool RESUME = false>
__device__ __forceinline__ void rs_solve_body(const uint32_t *__restrict__ tab, const uint64_t *__restrict__ desc, const RsTree *tree, const uint32_t *tree_of,
                                              uint32_t nmax, uint32_t Dmax, const RsSpots &spots, const RsOut &out, char *ws, uint32_t iters, uint32_t m,
                                              const RsLock &lk = RsLock{}, const RsResolve &rz = RsResolve{}, const RsResume &rm = RsResume{}) {
    static_assert(PER_SPOT || !LOCK, "the locked call has the tree-per-spot form only");
    static_assert(LOCK || !RESOLVE, "the re-solving call is the locked call with more arguments");
    static_assert(RESOLVE || !RESUME, "the resuming call is the re-solving call with more arguments");
    __shared__ uint32_t T[EVAL7_TAB_WORDS];
    __shared__ uint64_t slot[RS_SLOTS];               // key << 11 | pool holding, sorted once per spot; all ones = no holding.  After the
                                                      // sort the same memory holds rs and posof (below)
    __shared__ uint64_t pre[RS_PREFIX];               // pre[i]: both players' reach at sorted positions 0 .. i - 1
    __shared__ uint64_t pool[64];                     // card j of the pool (canonical order) as its bit in the suit-lane layout
    __shared__ uint32_t canon[64];                    // ... and its canonical index
    __shared__ uint64_t wsum[RS_WAVES];
    __shared__ RsTree tr;
    uint64_t *const rs = slot;                                                   // [RS_SORTED] a terminal's reaches in sorted order
    uint16_t *const posof = reinterpret_cast<uint16_t *>(slot + RS_SORTED);      // [RS_SORTED] pool holding -> its sorted position
    static_assert(RS_SORTED * 8 + RS_SORTED * 2 <= RS_SLOTS * 8, "rs and posof fit the sort slots");
    stage_eval7_tab<RS_BLOCK>(T, tab);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = uniform(tid >> 6);
    uint32_t n = 0, pot = 0, D = 0;
    int64_t *R = nullptr, *A = nullptr, *U0 = nullptr, *U1 = nullptr;
    uint64_t *RR = nullptr;
    uint32_t *SG = nullptr;
    // A tree into LDS (every lane of the workgroup comes here), and the workgroup's slice of the work space laid out for it
    auto stage = [&](const RsTree *src) {
        for (uint32_t w = tid; w < (uint32_t)(sizeof(RsTree) / 4); w += RS_BLOCK)
            reinterpret_cast<uint32_t *>(&tr)[PK_IDX(w, sizeof(RsTree) / 4, "tree")] = reinterpret_cast<const uint32_t *>(src)[w];
        __syncthreads();
        n = uniform(tr.n); pot = uniform(tr.pot);
        uint32_t dec = 0;
        for (uint32_t v = 0; v < n; ++v) dec += tr.kind[PK_IDX(v, RS_MAX_NODES, "kind")] <= RS_P1 ? 1u : 0u;
        D = uniform(dec);
        // the workgroup's slice of the work space, every array [n][RS_SORTED]
        char *const base = ws + (size_t)blockIdx.x * rs_group_bytes(PER_SPOT ? nmax : n);
        const size_t plane = (size_t)n * RS_SORTED;
        R = reinterpret_cast<int64_t *>(base); A = R + plane; U0 = A + plane; U1 = U0 + plane;
        RR = reinterpret_cast<uint64_t *>(U1 + plane);
        SG = reinterpret_cast<uint32_t *>(RR + plane);
    };
    if constexpr (!PER_SPOT) stage(tree);
    auto at = [&](uint32_t node, uint32_t i) -> size_t { return (size_t)PK_IDX(node, n, "node") * RS_SORTED + PK_IDX(i, RS_SORTED, "position"); };
    // a decision node's children (every lane of the wave asks together: the answer is wave-uniform); the slots past nact: node 0, never used
    auto kids = [&](uint32_t node, uint32_t nact, uint32_t (&ch)[4]) {
#pragma unroll
        for (int a = 0; a < 4; ++a) ch[a] = (uint32_t)a < nact ? uniform((uint32_t)tr.child[PK_IDX(node, RS_MAX_NODES, "child")][a]) : 0u;
    };

    for (uint32_t spot = blockIdx.x; spot < m; spot += gridDim.x) {
        __syncthreads();                              // (the table and the tree; the spot before: its pool and positions are done with)
        const uint64_t *d = desc + (size_t)spot * RS_DESC_WORDS;
        const uint64_t known = uniform(d[0]), meta = uniform(d[2]);
        const bool good = ((uint32_t)meta & 1u) != 0u;
        const uint64_t avail = good ? uniform(d[1]) : 0ull;     // (a refused spot: no holding is valid, every output is 0)
        const uint32_t P = (uint32_t)(meta >> 56);
        if constexpr (PER_SPOT) {
            // (good: k_trees_prep has seen tree_of[spot] < ntrees.  A refused spot stages tree 0, which always exists, and uses none of it:
            // staging on every path keeps n, pot and the slice's pointers plain values of the spot, not merges with the spot before)
            if constexpr (LOCK) stage(tree + ((good && tree_of) ? PK_IDX(uniform(tree_of[spot]), RS_MAX_TREES, "tree_of") : 0u));
            else stage(tree + (good ? PK_IDX(uniform(tree_of[spot]), RS_MAX_TREES, "tree_of") : 0u));
            if (!good) D = 0;
        }
        const uint32_t DS = PER_SPOT ? Dmax : D;      // the row stride of `strategy`
        // ---- the iterations the spot's state holds; fresh: a solved spot that starts from nothing, whose unread state entries become 0
        uint32_t t0 = 0;
        bool fresh = false;
        if constexpr (RESUME) {
            t0 = (good && rm.t0) ? uniform(rm.t0[spot]) : 0u;
            fresh = good && t0 == 0u;
        }
        // ---- zeros: every output at the holdings that are not in the pool, by the lanes of the fixed index h = tid + 512 j
        for (uint32_t h = tid; h < (uint32_t)RS_HOLDINGS; h += RS_BLOCK) {
            uint32_t ca = 0, cb = 1;
            unpair(h, ca, cb);
            if ((avail >> ca) & (avail >> cb) & 1ull) continue;
            for (uint32_t p = 0; p < 2u; ++p) {
                if (out.value) out.value[((size_t)spot * 2 + p) * RS_HOLDINGS + h] = 0;
                if (out.br) out.br[((size_t)spot * 2 + p) * RS_HOLDINGS + h] = 0;
                if constexpr (RESOLVE) {
                    if (rz.node_reach) rz.node_reach[((size_t)spot * 2 + p) * RS_HOLDINGS + h] = 0;
                    if (rz.node_value) rz.node_value[((size_t)spot * 2 + p) * RS_HOLDINGS + h] = 0;
                    if (rz.node_br) rz.node_br[((size_t)spot * 2 + p) * RS_HOLDINGS + h] = 0;
                }
            }
            if (out.strategy)
                for (uint32_t r = 0; r < DS * 4u; ++r) out.strategy[((size_t)spot * DS * 4 + r) * RS_HOLDINGS + h] = 0;
            if constexpr (RESUME)
                if (fresh)
                    for (uint32_t r = 0; r < DS * 4u; ++r) {
                        rm.regret[((size_t)spot * DS * 4 + r) * RS_HOLDINGS + h] = 0;
                        rm.average[((size_t)spot * DS * 4 + r) * RS_HOLDINGS + h] = 0;
                    }
        }
        // ... and, where the call's stride is wider than the spot's tree, the rows past its own at the holdings of the pool
        if constexpr (PER_SPOT)
            if (out.strategy && D < DS)
                for (uint32_t h = tid; h < (uint32_t)RS_HOLDINGS; h += RS_BLOCK) {
                    uint32_t ca = 0, cb = 1;
                    unpair(h, ca, cb);
                    if (!((avail >> ca) & (avail >> cb) & 1ull)) continue;
                    for (uint32_t r = D * 4u; r < DS * 4u; ++r) out.strategy[((size_t)spot * DS * 4 + r) * RS_HOLDINGS + h] = 0;
                }
        if constexpr (RESUME)
            if (fresh && D < DS)
                for (uint32_t h = tid; h < (uint32_t)RS_HOLDINGS; h += RS_BLOCK) {
                    uint32_t ca = 0, cb = 1;
                    unpair(h, ca, cb);
                    if (!((avail >> ca) & (avail >> cb) & 1ull)) continue;
                    for (uint32_t r = D * 4u; r < DS * 4u; ++r) {
                        rm.regret[((size_t)spot * DS * 4 + r) * RS_HOLDINGS + h] = 0;
                        rm.average[((size_t)spot * DS * 4 + r) * RS_HOLDINGS + h] = 0;
                    }
                }
        if (!good) continue;
        fill_pool(pool, canon, avail, tid);
        __syncthreads();
        const uint32_t nh = tri(P);
        uint32_t npad = 64;
        while (npad < nh) npad <<= 1;                 // (> nh: C(P, 2) is no power of two for P >= 3, so a pad slot always exists)
        // ---- rank: every pool holding once, on the complete board
        for (uint32_t ph = tid; ph < npad; ph += RS_BLOCK) {
            uint64_t s = ~0ull;
            if (ph < nh) {
                uint32_t ea, eb;
                unpair(ph, ea, eb);
                const uint64_t bits = known | pool[PK_IDX(ea, 64, "pool")] | pool[PK_IDX(eb, 64, "pool")];
                s = ((uint64_t)order_key(eval7_tab_back(eval7_tab_front_bits(bits, T), T)) << 11) | ph;
            }
            slot[PK_IDX(ph, RS_SLOTS, "slot")] = s;
        }
        __syncthreads();
        // ---- order: bitonic sort of slot[0 .. npad), ascending
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
        // ---- the positions this lane owns: the holding there (pool slots ha < hb, fixed index gh) and the bounds of its key
        uint32_t ha[RS_PER_LANE], hb[RS_PER_LANE], gh[RS_PER_LANE], lb[RS_PER_LANE], ub[RS_PER_LANE], hph[RS_PER_LANE];
#pragma unroll
        for (int j = 0; j < RS_PER_LANE; ++j) {
            const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
            ha[j] = 0; hb[j] = 1; gh[j] = 0; lb[j] = 0; ub[j] = 0; hph[j] = 0;
            if (i < nh) {
                const uint64_t s = slot[PK_IDX(i, RS_SLOTS, "slot")];
                const uint32_t kh = (uint32_t)(s >> 11);
                hph[j] = (uint32_t)s & 2047u;
                unpair(hph[j], ha[j], hb[j]);
                gh[j] = tri(canon[PK_IDX(hb[j], 64, "canon")]) + canon[PK_IDX(ha[j], 64, "canon")];
                uint32_t l = 0, u = 0;                                          // sorted positions with a key < kh, <= kh
                for (uint32_t step = npad >> 1; step > 0; step >>= 1) {
                    const uint32_t kl = (uint32_t)(slot[PK_IDX(l + step - 1u, RS_SLOTS, "slot")] >> 11);
                    const uint32_t ku = (uint32_t)(slot[PK_IDX(u + step - 1u, RS_SLOTS, "slot")] >> 11);
                    l += kl < kh ? step : 0u;
                    u += ku <= kh ? step : 0u;
                }
                lb[j] = l; ub[j] = u;
            }
        }
        __syncthreads();                              // (the slots have been read: their memory becomes rs and posof)
#pragma unroll
        for (int j = 0; j < RS_PER_LANE; ++j) {
            const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
            if (i < nh) posof[PK_IDX(hph[j], RS_SORTED, "posof")] = (uint16_t)i;
        }
        // ---- the root's reaches; regrets and accumulators start at 0
        const uint16_t *w0 = spots.ranges + (size_t)spot * 2 * RS_HOLDINGS, *w1 = w0 + RS_HOLDINGS;
#pragma unroll
        for (int j = 0; j < RS_PER_LANE; ++j) {
            const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
            if (i >= nh) continue;
            if constexpr (RESOLVE) {
                if (rz.reach) {                       // (the solver's own units: no shift, the bound of a shifted weight)
                    const uint32_t *q = rz.reach + (size_t)spot * 2 * RS_HOLDINGS + PK_IDX(gh[j], RS_HOLDINGS, "reach");
                    const uint32_t q0 = q[0], q1 = q[RS_HOLDINGS];
                    RR[at(0, i)] = (uint64_t)(q0 < RS_REACH_MAX ? q0 : RS_REACH_MAX) | ((uint64_t)(q1 < RS_REACH_MAX ? q1 : RS_REACH_MAX) << 32);
                } else RR[at(0, i)] = ((uint64_t)w0[PK_IDX(gh[j], RS_HOLDINGS, "range")] << 4) | ((uint64_t)w1[PK_IDX(gh[j], RS_HOLDINGS, "range")] << 36);
            } else {
                RR[at(0, i)] = ((uint64_t)w0[PK_IDX(gh[j], RS_HOLDINGS, "range")] << 4) | ((uint64_t)w1[PK_IDX(gh[j], RS_HOLDINGS, "range")] << 36);
            }
            for (uint32_t v = 1; v < n; ++v) { R[at(v, i)] = 0; A[at(v, i)] = 0; }
        }
        // ---- the locked nodes of the spot (bit v: decision node v), and their probabilities into SG: the rule on the caller's weights
        uint64_t lockm = 0;
        if constexpr (LOCK) {
            if (lk.lock)
                for (uint32_t v = 0; v < n; ++v) {
                    if (tr.kind[PK_IDX(v, RS_MAX_NODES, "kind")] > RS_P1) continue;
                    const uint32_t row = tr.row[PK_IDX(v, RS_MAX_NODES, "row")];
                    lockm |= lk.lock[(size_t)spot * Dmax + PK_IDX(row, Dmax, "lock row")] ? 1ull << v : 0ull;
                }
            lockm = uniform(lockm);
            for (uint32_t node = 0; node < n; ++node) {
                if (!((lockm >> node) & 1ull)) continue;
                const uint32_t nact = uniform((uint32_t)tr.nact[PK_IDX(node, RS_MAX_NODES, "nact")]), row = uniform((uint32_t)tr.row[PK_IDX(node, RS_MAX_NODES, "row")]);
                uint32_t ch[4];
                kids(node, nact, ch);
                const uint16_t *src = lk.locked + ((size_t)spot * Dmax + row) * 4 * RS_HOLDINGS;
#pragma unroll
                for (int j = 0; j < RS_PER_LANE; ++j) {
                    const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                    if (i >= nh) continue;
                    int64_t X[4];
                    uint32_t sig[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) X[a] = (uint32_t)a < nact ? (int64_t)src[(size_t)a * RS_HOLDINGS + PK_IDX(gh[j], RS_HOLDINGS, "locked")] : 0;
                    rs_sigma(X, nact, sig);
#pragma unroll
                    for (int a = 0; a < 4; ++a)
                        if ((uint32_t)a < nact) SG[at(ch[a], i)] = sig[a];
                }
            }
        }
        auto locked_at = [&](uint32_t node) -> bool { return LOCK && ((lockm >> node) & 1ull) != 0ull; };
        // ---- a resumed spot: R and A of its free rows from the caller's state, by the owner of each position
        if constexpr (RESUME)
            if (t0 > 0u)
                for (uint32_t node = 0; node < n; ++node) {
                    if (uniform((uint32_t)tr.kind[PK_IDX(node, RS_MAX_NODES, "kind")]) > RS_P1 || locked_at(node)) continue;
                    const uint32_t nact = uniform((uint32_t)tr.nact[PK_IDX(node, RS_MAX_NODES, "nact")]), row = uniform((uint32_t)tr.row[PK_IDX(node, RS_MAX_NODES, "row")]);
                    uint32_t ch[4];
                    kids(node, nact, ch);
                    const size_t o = ((size_t)spot * DS + PK_IDX(row, DS, "state row")) * 4 * RS_HOLDINGS;
#pragma unroll
                    for (int j = 0; j < RS_PER_LANE; ++j) {
                        const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                        if (i >= nh) continue;
#pragma unroll
                        for (int a = 0; a < 4; ++a) {
                            if ((uint32_t)a >= nact) continue;
                            const size_t g = o + (size_t)a * RS_HOLDINGS + PK_IDX(gh[j], RS_HOLDINGS, "state");
                            const int64_t r = rm.regret[g], v = rm.average[g];
                            R[at(ch[a], i)] = r < 0 ? 0 : r > RS_RESUME_RMAX ? RS_RESUME_RMAX : r;
                            A[at(ch[a], i)] = v < 0 ? 0 : v > RS_RESUME_AMAX ? RS_RESUME_AMAX : v;
                        }
                    }
                }
        __syncthreads();                              // (posof)

        // A terminal node: both players' values of every holding from the opponent's reaches (every lane of the workgroup comes here)
        auto terminal = [&](uint32_t node, uint32_t kind) {
            if constexpr (RESOLVE)
                if (kind == (uint32_t)RS_GIVEN) {     // the caller's values, whatever the reaches: no order, no sum, no LDS
#pragma unroll
                    for (int j = 0; j < RS_PER_LANE; ++j) {
                        const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                        if (i >= nh) continue;
                        const int64_t *g = rz.given + (size_t)spot * 2 * RS_HOLDINGS + PK_IDX(gh[j], RS_HOLDINGS, "given");
                        const int64_t g0 = g[0], g1 = g[RS_HOLDINGS];
                        U0[at(node, i)] = g0 > RS_GIVEN_MAX ? RS_GIVEN_MAX : g0 < -RS_GIVEN_MAX ? -RS_GIVEN_MAX : g0;
                        U1[at(node, i)] = g1 > RS_GIVEN_MAX ? RS_GIVEN_MAX : g1 < -RS_GIVEN_MAX ? -RS_GIVEN_MAX : g1;
                    }
                    return;
                }
#pragma unroll
            for (int j = 0; j < RS_PER_LANE; ++j) {
                const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                if (i < nh) rs[PK_IDX(i, RS_SORTED, "rs")] = RR[at(node, i)];
            }
            __syncthreads();
            // exclusive prefix sum in sorted order: three positions per lane, a wave scan, the waves' totals
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
            const uint32_t f = kind - RS_FOLD0, pf = tr.put[PK_IDX(node, RS_MAX_NODES, "put")][f & 1u], c = tr.put[PK_IDX(node, RS_MAX_NODES, "put")][0];
#pragma unroll
            for (int j = 0; j < RS_PER_LANE; ++j) {
                const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                if (i >= nh) continue;
                const uint64_t below0 = pre[PK_IDX(lb[j], RS_PREFIX, "pre")], self = rs[PK_IDX(i, RS_SORTED, "rs")];
                uint64_t below = below0, equal = pre[PK_IDX(ub[j], RS_PREFIX, "pre")] - below0 - self, conf = self;
                // card removal: every holding {ha, x}, {hb, x}, by its own sorted position
                const uint32_t ta = tri(ha[j]), tb = tri(hb[j]);
                // (no branch in the loop, so that the loads of several x are in flight together: x = ha or hb looks h itself up and counts 0)
#pragma unroll 4
                for (uint32_t x = 0; x < P; ++x) {
                    const bool own = x == ha[j] || x == hb[j];
                    const uint32_t tx = tri(x);
                    const uint32_t i0 = own ? hph[j] : pair(ha[j], ta, x, tx), i1 = own ? hph[j] : pair(hb[j], tb, x, tx);
                    const uint32_t p0 = posof[PK_IDX(i0, RS_SORTED, "posof")], p1 = posof[PK_IDX(i1, RS_SORTED, "posof")];
                    const uint64_t r0 = own ? 0ull : rs[PK_IDX(p0, RS_SORTED, "rs")], r1 = own ? 0ull : rs[PK_IDX(p1, RS_SORTED, "rs")];
                    conf += r0 + r1;
                    below -= (p0 < lb[j] ? r0 : 0ull) + (p1 < lb[j] ? r1 : 0ull);
                    equal -= ((p0 >= lb[j] && p0 < ub[j]) ? r0 : 0ull) + ((p1 >= lb[j] && p1 < ub[j]) ? r1 : 0ull);
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
                U0[at(node, i)] = u0;
                U1[at(node, i)] = u1;
            }
            __syncthreads();                          // (rs, pre and the totals are rewritten by the next terminal)
        };

        // One walk down: reaches, and every terminal's values.  FROM_R: the probabilities come from the regrets and are kept in SG;
        // otherwise SG is played as it stands.
        auto down = [&](bool walk_from_r) {
            for (uint32_t node = 0; node < n; ++node) {
                const uint32_t kind = uniform((uint32_t)tr.kind[PK_IDX(node, RS_MAX_NODES, "kind")]);
                if (kind > RS_P1) { terminal(node, kind); continue; }
                const bool from_r = walk_from_r && !locked_at(node);          // (a locked node: SG holds what is played there)
                const uint32_t nact = uniform((uint32_t)tr.nact[PK_IDX(node, RS_MAX_NODES, "nact")]);
                uint32_t ch[4];
                kids(node, nact, ch);
#pragma unroll
                for (int j = 0; j < RS_PER_LANE; ++j) {
                    const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                    if (i >= nh) continue;
                    uint32_t sig[4];
                    if (from_r) {
                        int64_t X[4];
#pragma unroll
                        for (int a = 0; a < 4; ++a) X[a] = (uint32_t)a < nact ? R[at(ch[a], i)] : 0;
                        rs_sigma(X, nact, sig);
                    }
                    const uint64_t rr = RR[at(node, i)];
                    const uint32_t r0 = (uint32_t)rr, r1 = (uint32_t)(rr >> 32);
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        if ((uint32_t)a >= nact) continue;
                        const size_t e = at(ch[a], i);
                        if (from_r) SG[e] = sig[a]; else sig[a] = SG[e];
                        const uint32_t mine = (uint32_t)(((uint64_t)(kind == RS_P0 ? r0 : r1) * sig[a]) >> 15);
                        RR[e] = kind == RS_P0 ? ((uint64_t)mine | ((uint64_t)r1 << 32)) : ((uint64_t)r0 | ((uint64_t)mine << 32));
                    }
                }
            }
        };

        // ---- the iterations: one walk down, then the walk up with the regret and accumulator updates of each decision node
        for (uint32_t t = 1; t <= iters; ++t) {
            const uint32_t tw = RESUME ? t0 + t : t;  // (the iteration's number: all that t enters is the accumulators' weight)
            down(true);
            for (uint32_t node = n; node-- > 0u;) {
                const uint32_t kind = uniform((uint32_t)tr.kind[PK_IDX(node, RS_MAX_NODES, "kind")]);
                if (kind > RS_P1) continue;
                const uint32_t nact = uniform((uint32_t)tr.nact[PK_IDX(node, RS_MAX_NODES, "nact")]);
                int64_t *const Up = kind == RS_P0 ? U0 : U1, *const Uq = kind == RS_P0 ? U1 : U0;
                uint32_t ch[4];
                kids(node, nact, ch);
#pragma unroll
                for (int j = 0; j < RS_PER_LANE; ++j) {
                    const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                    if (i >= nh) continue;
                    int64_t up[4], acc = 0, uq = 0;
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        up[a] = 0;
                        if ((uint32_t)a >= nact) continue;
                        const size_t e = at(ch[a], i);
                        up[a] = Up[e];
                        acc += (int64_t)SG[e] * up[a];
                        uq += Uq[e];
                    }
                    const int64_t un = acc >> 15;     // (the sum first, the floor once)
                    Up[at(node, i)] = un;
                    Uq[at(node, i)] = uq;
                    if (locked_at(node)) continue;    // (neither R nor A is updated at a locked node)
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        if ((uint32_t)a >= nact) continue;
                        const size_t e = at(ch[a], i);
                        const int64_t r = R[e] + up[a] - un;
                        R[e] = r > 0 ? r : 0;
                        const uint64_t rr = RR[e];
                        A[e] += (int64_t)((uint64_t)tw * (uint64_t)(kind == RS_P0 ? (uint32_t)rr : (uint32_t)(rr >> 32)));
                    }
                }
            }
        }

        // ---- the state goes back to the caller: R and A as they stand at the free rows; at a locked row and at the action slots past nact a
        // fresh spot writes 0, a resumed one nothing
        if constexpr (RESUME)
            for (uint32_t node = 0; node < n; ++node) {
                if (uniform((uint32_t)tr.kind[PK_IDX(node, RS_MAX_NODES, "kind")]) > RS_P1) continue;
                const bool locked = locked_at(node);
                if (locked && !fresh) continue;
                const uint32_t nact = uniform((uint32_t)tr.nact[PK_IDX(node, RS_MAX_NODES, "nact")]), row = uniform((uint32_t)tr.row[PK_IDX(node, RS_MAX_NODES, "row")]);
                uint32_t ch[4];
                kids(node, nact, ch);
                const size_t o = ((size_t)spot * DS + PK_IDX(row, DS, "state row")) * 4 * RS_HOLDINGS;
#pragma unroll
                for (int j = 0; j < RS_PER_LANE; ++j) {
                    const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                    if (i >= nh) continue;
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const bool live = (uint32_t)a < nact && !locked;
                        if (!(live || fresh)) continue;
                        const size_t g = o + (size_t)a * RS_HOLDINGS + PK_IDX(gh[j], RS_HOLDINGS, "state");
                        rm.regret[g] = live ? R[at(ch[a], i)] : 0;
                        rm.average[g] = live ? A[at(ch[a], i)] : 0;
                    }
                }
            }

        // ---- the average strategy: the rule applied to the accumulators; it stays in SG for the last walk
        for (uint32_t node = 0; node < n; ++node) {
            const uint32_t kind = uniform((uint32_t)tr.kind[PK_IDX(node, RS_MAX_NODES, "kind")]);
            if (kind > RS_P1) continue;
            const uint32_t nact = uniform((uint32_t)tr.nact[PK_IDX(node, RS_MAX_NODES, "nact")]), row = uniform((uint32_t)tr.row[PK_IDX(node, RS_MAX_NODES, "row")]);
            uint32_t ch[4];
            kids(node, nact, ch);
#pragma unroll
            for (int j = 0; j < RS_PER_LANE; ++j) {
                const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                if (i >= nh) continue;
                int64_t X[4];
                uint32_t sig[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) X[a] = (uint32_t)a < nact ? A[at(ch[a], i)] : 0;
                if (locked_at(node)) {
#pragma unroll
                    for (int a = 0; a < 4; ++a) sig[a] = (uint32_t)a < nact ? SG[at(ch[a], i)] : 0u;
                } else rs_sigma(X, nact, sig);
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    if ((uint32_t)a < nact) SG[at(ch[a], i)] = sig[a];
                    if (out.strategy) out.strategy[(((size_t)spot * DS + row) * 4 + (uint32_t)a) * RS_HOLDINGS + gh[j]] = (uint16_t)sig[a];
                }
            }
        }
        // (RESOLVE: written as two statements, and without a flag of its own, so that the other instantiations compile as they did)
        if constexpr (RESOLVE) {
            if (!(out.value || out.br || rz.node_reach || rz.node_value || rz.node_br)) continue;
        } else {
            if (!(out.value || out.br)) continue;
        }
        // ---- its values and the best responses against it: the walk up carries, beside each player's value, the value of the player
        // who plays the maximum at its own nodes (B0 / B1, in the memory of R / A; a terminal's is its value)
        down(false);
        for (uint32_t node = n; node-- > 0u;) {
            const uint32_t kind = uniform((uint32_t)tr.kind[PK_IDX(node, RS_MAX_NODES, "kind")]);
            if (kind > RS_P1) continue;
            const uint32_t nact = uniform((uint32_t)tr.nact[PK_IDX(node, RS_MAX_NODES, "nact")]);
            int64_t *const Up = kind == RS_P0 ? U0 : U1, *const Uq = kind == RS_P0 ? U1 : U0;
            int64_t *const Bp = kind == RS_P0 ? R : A, *const Bq = kind == RS_P0 ? A : R;
            uint32_t ch[4];
            bool leaf[4];
            kids(node, nact, ch);
#pragma unroll
            for (int a = 0; a < 4; ++a) leaf[a] = uniform((uint32_t)tr.kind[PK_IDX(ch[a], RS_MAX_NODES, "kind")]) > RS_P1;
#pragma unroll
            for (int j = 0; j < RS_PER_LANE; ++j) {
                const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                if (i >= nh) continue;
                int64_t acc = 0, uq = 0, bp = 0, bq = 0;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    if ((uint32_t)a >= nact) continue;
                    const size_t e = at(ch[a], i);
                    const int64_t up = Up[e], uqa = Uq[e], bpa = leaf[a] ? up : Bp[e], bqa = leaf[a] ? uqa : Bq[e];
                    acc += (int64_t)SG[e] * up;
                    uq += uqa;
                    bp = (a == 0 || bpa > bp) ? bpa : bp;
                    bq += bqa;
                }
                Up[at(node, i)] = acc >> 15;
                Uq[at(node, i)] = uq;
                Bp[at(node, i)] = bp;
                Bq[at(node, i)] = bq;
            }
        }
#pragma unroll
        for (int j = 0; j < RS_PER_LANE; ++j) {
            const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
            if (i >= nh) continue;
            const size_t o = (size_t)spot * 2 * RS_HOLDINGS + gh[j];
            if (out.value) { out.value[o] = U0[at(0, i)]; out.value[o + RS_HOLDINGS] = U1[at(0, i)]; }
            if (out.br) { out.br[o] = R[at(0, i)]; out.br[o + RS_HOLDINGS] = A[at(0, i)]; }
        }
        if constexpr (RESOLVE)
            if (rz.node_reach || rz.node_value || rz.node_br) {
                const uint32_t an = uniform((uint32_t)rz.at[spot]);
                const bool leaf = uniform((uint32_t)tr.kind[PK_IDX(an, RS_MAX_NODES, "kind")]) > RS_P1;      // (a terminal's best response is its value)
#pragma unroll
                for (int j = 0; j < RS_PER_LANE; ++j) {
                    const uint32_t i = tid + (uint32_t)j * RS_BLOCK;
                    if (i >= nh) continue;
                    const size_t o = (size_t)spot * 2 * RS_HOLDINGS + gh[j], e = at(an, i);
                    if (rz.node_reach) { const uint64_t rr = RR[e]; rz.node_reach[o] = (uint32_t)rr; rz.node_reach[o + RS_HOLDINGS] = (uint32_t)(rr >> 32); }
                    if (rz.node_value) { rz.node_value[o] = U0[e]; rz.node_value[o + RS_HOLDINGS] = U1[e]; }
                    if (rz.node_br) { rz.node_br[o] = leaf ? U0[e] : R[e]; rz.node_br[o + RS_HOLDINGS] = leaf ? U1[e] : A[e]; }
                }
            }
    }
}

// registers: one workgroup per CU is two waves per SIMD
__global__ void __launch_bounds__(RS_BLOCK, 2) k_river_solve(const uint32_t *__restrict__ tab, const uint64_t *__restrict__ desc, RsTree tree, RsSpots spots,
                                                             RsOut out, char *ws, uint32_t iters, uint32_t m) {
    rs_solve_body<false>(tab, desc, &tree, nullptr, 0u, 0u, spots, out, ws, iters, m);
}
__global__ void __launch_bounds__(RS_BLOCK, 2) k_trees_river_solve(const uint32_t *__restrict__ tab, const uint64_t *__restrict__ desc, RsTrees trees, RsSpots spots,
                                                                   RsOut out, char *ws, uint32_t iters, uint32_t m) {
    rs_solve_body<true>(tab, desc, trees.trees, trees.tree_of, trees.nmax, trees.Dmax, spots, out, ws, iters, m);
}

// the locked call: k_trees_river_solve's body with LOCK (the name does not begin with k_river_solve or k_trees_: host tests list those)
__global__ void __launch_bounds__(RS_BLOCK, 2) k_lock_river_solve(const uint32_t *__restrict__ tab, const uint64_t *__restrict__ desc, RsTrees trees, RsLock lk,
                                                                  RsSpots spots, RsOut out, char *ws, uint32_t iters, uint32_t m) {
    rs_solve_body<true, true>(tab, desc, trees.trees, trees.tree_of, trees.nmax, trees.Dmax, spots, out, ws, iters, m, lk);
}

// the re-solving call: k_lock_river_solve's body with RESOLVE (the name begins with none of the prefixes host tests list kernels by)
__global__ void __launch_bounds__(RS_BLOCK, 2) k_resolve_river_solve(const uint32_t *__restrict__ tab, const uint64_t *__restrict__ desc, RsTrees trees, RsLock lk,
                                                                     RsResolve rz, RsSpots spots, RsOut out, char *ws, uint32_t iters, uint32_t m) {
    rs_solve_body<true, true, true>(tab, desc, trees.trees, trees.tree_of, trees.nmax, trees.Dmax, spots, out, ws, iters, m, lk, rz);
}

// the resuming call: k_resolve_river_solve's body with RESUME (the name begins with none of the prefixes host tests list kernels by)
__global__ void __launch_bounds__(RS_BLOCK, 2) k_resume_river_solve(const uint32_t *__restrict__ tab, const uint64_t *__restrict__ desc, RsTrees trees, RsLock lk,
                                                                    RsResolve rz, RsResume rm, RsSpots spots, RsOut out, char *ws, uint32_t iters, uint32_t m) {
    rs_solve_body<true, true, true, true>(tab, desc, trees.trees, trees.tree_of, trees.nmax, trees.Dmax, spots, out, ws, iters, m, lk, rz, rm);
}

// The last part of a resuming call's preparation (pk_river_solver.hpp): one lane per spot, only spots that are still good are judged
__global__ void __launch_bounds__(RS_PREP_BLOCK) k_resume_prep(const uint32_t *__restrict__ t0, uint32_t iters, uint64_t *desc, uint8_t *status, size_t m) {
    const size_t i = (size_t)blockIdx.x * RS_PREP_BLOCK + threadIdx.x;
    if (i >= m) return;
    uint64_t *d = desc + i * (size_t)RS_DESC_WORDS;
    if (!(d[2] & 1ull) || (uint64_t)t0[i] + iters <= (uint64_t)RS_MAX_ITERS) return;
    d[2] &= ~1ull;
    if (status) status[i] |= (uint8_t)PK_EQ_BAD_ITER;
}

// The last part of a re-solving call's preparation (pk_river_solver.hpp): one lane per spot, only spots that are still good are judged
struct ResolvePrepArgs {
    const char *trees;
    uint32_t stride, river_off;
    const uint32_t *tree_of;
    const uint8_t *at, *at_card;
    uint64_t *desc;
    uint8_t *status;
    size_t m;
};
__global__ void __launch_bounds__(RS_PREP_BLOCK) k_resolve_prep(ResolvePrepArgs a) {
    const size_t i = (size_t)blockIdx.x * RS_PREP_BLOCK + threadIdx.x;
    if (i >= a.m) return;
    uint64_t *d = a.desc + i * (size_t)RS_DESC_WORDS;
    if (!(d[2] & 1ull)) return;                       // (refused before: its tree_of may name no tree)
    const char *t = a.trees + (size_t)(a.tree_of ? a.tree_of[i] : 0u) * a.stride;
    const uint32_t n = *reinterpret_cast<const uint32_t *>(t), node = a.at[i];
    uint32_t bad = 0;
    if (node >= n) bad = PK_EQ_BAD_TREE;
    else if (a.river_off && reinterpret_cast<const uint8_t *>(t)[a.river_off + node]) {
        const uint32_t c = a.at_card ? a.at_card[i] : 0xFFu;
        if (c >= 0x40u || (c & 15u) >= 13u || !((d[1] >> ((c & 15u) * 4u + (c >> 4))) & 1ull)) bad = PK_EQ_BAD_CARD;
    }
    if (!bad) return;
    d[2] &= ~1ull;
    if (a.status) a.status[i] |= (uint8_t)bad;
}

namespace pk {

hipError_t rs_launch(hipStream_t stream, const uint32_t *tab, const RsSpots &spots, const RsTree &tree, uint32_t iters, size_t m, const RsOut &out,
                     char *work) {
    if (m == 0) return hipSuccess;
    const RsPrepArgs a{spots, out.status, (uint64_t *)work, m};
    hipLaunchKernelGGL(k_rs_prep, dim3((unsigned)((m + RS_PREP_BLOCK - 1) / RS_PREP_BLOCK)), dim3(RS_PREP_BLOCK), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !(out.strategy || out.value || out.br)) return e;   // (status alone: the preparation kernel has written it)
    hipLaunchKernelGGL(k_river_solve, dim3(rs_grid(m)), dim3(RS_BLOCK), 0, stream, tab, (const uint64_t *)work, tree, spots, out, work + rs_desc_bytes(m),
                       iters, (uint32_t)m);
    return hipGetLastError();
}

hipError_t trees_prep_launch(hipStream_t stream, const uint32_t *tree_of, uint32_t ntrees, uint64_t *desc, uint8_t *status, size_t m) {
    hipLaunchKernelGGL(k_trees_prep, dim3((unsigned)((m + RS_PREP_BLOCK - 1) / RS_PREP_BLOCK)), dim3(RS_PREP_BLOCK), 0, stream, tree_of, ntrees, desc, status, m);
    return hipGetLastError();
}

hipError_t rs_launch_trees(hipStream_t stream, const uint32_t *tab, const RsSpots &spots, const RsTrees &trees, uint32_t ntrees, uint32_t iters, size_t m,
                           const RsOut &out, char *work) {
    if (m == 0) return hipSuccess;
    const RsPrepArgs a{spots, out.status, (uint64_t *)work, m};
    hipLaunchKernelGGL(k_rs_prep, dim3((unsigned)((m + RS_PREP_BLOCK - 1) / RS_PREP_BLOCK)), dim3(RS_PREP_BLOCK), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = trees_prep_launch(stream, trees.tree_of, ntrees, (uint64_t *)work, out.status, m);
    if (e != hipSuccess || !(out.strategy || out.value || out.br)) return e;   // (status alone: the preparation kernel has written it)
    hipLaunchKernelGGL(k_trees_river_solve, dim3(rs_grid(m)), dim3(RS_BLOCK), 0, stream, tab, (const uint64_t *)work, trees, spots, out,
                       work + rs_desc_bytes(m), iters, (uint32_t)m);
    return hipGetLastError();
}

hipError_t rs_launch_locked(hipStream_t stream, const uint32_t *tab, const RsSpots &spots, const RsTrees &trees, uint32_t ntrees, const RsLock &lk,
                            uint32_t iters, size_t m, const RsOut &out, char *work) {
    if (m == 0) return hipSuccess;
    const RsPrepArgs a{spots, out.status, (uint64_t *)work, m};
    hipLaunchKernelGGL(k_rs_prep, dim3((unsigned)((m + RS_PREP_BLOCK - 1) / RS_PREP_BLOCK)), dim3(RS_PREP_BLOCK), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && trees.tree_of) e = trees_prep_launch(stream, trees.tree_of, ntrees, (uint64_t *)work, out.status, m);
    if (e != hipSuccess || !(out.strategy || out.value || out.br)) return e;   // (status alone: the preparation kernels have written it)
    hipLaunchKernelGGL(k_lock_river_solve, dim3(rs_grid(m)), dim3(RS_BLOCK), 0, stream, tab, (const uint64_t *)work, trees, lk, spots, out,
                       work + rs_desc_bytes(m), iters, (uint32_t)m);
    return hipGetLastError();
}

hipError_t resolve_prep_launch(hipStream_t stream, const void *trees, uint32_t stride, uint32_t river_off, const uint32_t *tree_of, const uint8_t *at,
                               const uint8_t *at_card, uint64_t *desc, uint8_t *status, size_t m) {
    const ResolvePrepArgs a{(const char *)trees, stride, river_off, tree_of, at, at_card, desc, status, m};
    hipLaunchKernelGGL(k_resolve_prep, dim3((unsigned)((m + RS_PREP_BLOCK - 1) / RS_PREP_BLOCK)), dim3(RS_PREP_BLOCK), 0, stream, a);
    return hipGetLastError();
}

hipError_t rs_launch_resolve(hipStream_t stream, const uint32_t *tab, const RsSpots &spots, const RsTrees &trees, uint32_t ntrees, const RsLock &lk,
                             const RsResolve &rz, uint32_t iters, size_t m, const RsOut &out, char *work) {
    if (m == 0) return hipSuccess;
    const RsPrepArgs a{spots, out.status, (uint64_t *)work, m};
    hipLaunchKernelGGL(k_rs_prep, dim3((unsigned)((m + RS_PREP_BLOCK - 1) / RS_PREP_BLOCK)), dim3(RS_PREP_BLOCK), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && trees.tree_of) e = trees_prep_launch(stream, trees.tree_of, ntrees, (uint64_t *)work, out.status, m);
    if (e == hipSuccess && rz.at) e = resolve_prep_launch(stream, trees.trees, (uint32_t)sizeof(RsTree), 0u, trees.tree_of, rz.at, nullptr, (uint64_t *)work, out.status, m);
    if (e != hipSuccess || !(out.strategy || out.value || out.br || rz.at)) return e;   // (status alone: the preparation kernels have written it)
    hipLaunchKernelGGL(k_resolve_river_solve, dim3(rs_grid(m)), dim3(RS_BLOCK), 0, stream, tab, (const uint64_t *)work, trees, lk, rz, spots, out,
                       work + rs_desc_bytes(m), iters, (uint32_t)m);
    return hipGetLastError();
}

hipError_t resume_prep_launch(hipStream_t stream, const uint32_t *t0, uint32_t iters, uint64_t *desc, uint8_t *status, size_t m) {
    hipLaunchKernelGGL(k_resume_prep, dim3((unsigned)((m + RS_PREP_BLOCK - 1) / RS_PREP_BLOCK)), dim3(RS_PREP_BLOCK), 0, stream, t0, iters, desc, status, m);
    return hipGetLastError();
}

hipError_t rs_launch_resume(hipStream_t stream, const uint32_t *tab, const RsSpots &spots, const RsTrees &trees, uint32_t ntrees, const RsLock &lk,
                            const RsResolve &rz, const RsResume &rm, uint32_t iters, size_t m, const RsOut &out, char *work) {
    if (m == 0) return hipSuccess;
    const RsPrepArgs a{spots, out.status, (uint64_t *)work, m};
    hipLaunchKernelGGL(k_rs_prep, dim3((unsigned)((m + RS_PREP_BLOCK - 1) / RS_PREP_BLOCK)), dim3(RS_PREP_BLOCK), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && trees.tree_of) e = trees_prep_launch(stream, trees.tree_of, ntrees, (uint64_t *)work, out.status, m);
    if (e == hipSuccess && rz.at) e = resolve_prep_launch(stream, trees.trees, (uint32_t)sizeof(RsTree), 0u, trees.tree_of, rz.at, nullptr, (uint64_t *)work, out.status, m);
    if (e == hipSuccess && rm.t0) e = resume_prep_launch(stream, rm.t0, iters, (uint64_t *)work, out.status, m);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_resume_river_solve, dim3(rs_grid(m)), dim3(RS_BLOCK), 0, stream, tab, (const uint64_t *)work, trees, lk, rz, rm, spots, out,
                       work + rs_desc_bytes(m), iters, (uint32_t)m);
    return hipGetLastError();
}

}  // namespace pk
