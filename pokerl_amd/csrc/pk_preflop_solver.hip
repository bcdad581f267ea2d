// pk_preflop_solver.hip -- the pre-flop solver (include/pokerl_hip.h "Pre-flop solver"): the river solver's simultaneous
// CFR+ (pk_river_solver.hip) on a game with no board, whose showdown is paid by the resident matchup table.  One kernel:
//   k_preflop_solve   a persistent grid of 512-thread workgroups, ONE SPOT PER WORKGROUP at a time, the spot's tree staged into LDS at its
//                     top from trees[tree_of[spot]] (tree_of NULL: tree 0).  There is no rank and no sort: every holding is valid, and a lane
//                     OWNS the holdings h = tid, tid + 512, tid + 1024 of the fixed index -- their regrets, average accumulators, reaches,
//                     probabilities and values, all in the workgroup's slice of the global work space, every word of which is read and
//                     written by its owner alone.  Only a terminal couples lanes: both players' reaches go to LDS as ONE 64-bit word
//                     (player 0 low, player 1 high: a half of S or of a card's sum stays below 2^31, and the sum of the 52 card sums, which holds every reach twice, below 2^32).  52 per-card sums give S(h) = total - the
//                     sums of h's two cards + its own entry, which is all a fold needs.  A showdown adds the integer mat-vec
//                     E(h) = sum over h' of reach[h'] * (2 win[h][h'] + tie[h][h']): a WAVE PER ROW, its lanes reading the row's win and
//                     tie words coalesced and both reach vectors from LDS (one pass over the matrix serves both players), a cross-lane
//                     sum, lane 0 storing the row's two sums in LDS; the owners then form floor((pot + 2c) E / B) - 2c S.
//                     The status (0 or PK_EQ_BAD_TREE) is written by the same launch; the final passes (the average strategy, its values,
//                     the best responses) run in it too, as the river solver's do.
// Ordinary vector stores and LDS loads / stores only; no atomics, no scratch memory (tests/test_preflop_solver_host.py reads the code object).
#include <hip/hip_runtime.h>

#include "pk_equity_common.hpp"
#include "pk_preflop_solver.hpp"
#include "pk_solver_common.hpp"

using namespace pk;

// floor((pot + 2c) E / B) without the 2^66 product: (pot + 2c) (E div B) + ((pot + 2c) (E mod B)) div B -- the same integer, every
// intermediate below 2^46 (pot + 2c < 2^14, E < 2^52, so E div B < 2^32 and (pot + 2c) (E mod B) < 2^35)
__device__ __forceinline__ int64_t ps_share(uint64_t E, uint32_t chips) {
    const uint64_t q = E / (uint64_t)PS_BOARDS, r = E - q * (uint64_t)PS_BOARDS;
    return (int64_t)((uint64_t)chips * q + ((uint64_t)chips * r) / (uint64_t)PS_BOARDS);
}

// registers: one workgroup per CU is two waves per SIMD
__global__ void __launch_bounds__(PS_BLOCK, 2) k_preflop_solve(const uint32_t *__restrict__ M, const uint16_t *__restrict__ ranges, RsTrees trees, uint32_t ntrees,
                                                                RsOut out, char *ws, uint32_t iters, uint32_t m) {
    __shared__ uint64_t rq[PS_STRIDE];                // a terminal's reaches by holding: player 0 low, player 1 high
    __shared__ uint64_t E0[PS_STRIDE], E1[PS_STRIDE]; // a showdown's sums against player 1's / player 0's reach, by holding
    __shared__ uint64_t cs[64];                       // per card: the reaches of the 51 holdings that hold it
    __shared__ RsTree tr;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = uniform(tid >> 6);
    const bool solve = out.strategy || out.value || out.br;
    // the holdings this lane owns and their cards (the same for every spot)
    uint32_t ha[PS_PER_LANE], hb[PS_PER_LANE];
#pragma unroll
    for (int j = 0; j < PS_PER_LANE; ++j) {
        const uint32_t h = tid + (uint32_t)j * PS_BLOCK;
        ha[j] = 0; hb[j] = 1;
        if (h < (uint32_t)RS_HOLDINGS) unpair(h, ha[j], hb[j]);
    }
    uint32_t n = 0, pot = 0, D = 0;
    int64_t *R = nullptr, *A = nullptr, *U0 = nullptr, *U1 = nullptr;
    uint64_t *RR = nullptr;
    uint32_t *SG = nullptr;
    auto at = [&](uint32_t node, uint32_t h) -> size_t { return (size_t)PK_IDX(node, n, "node") * PS_STRIDE + PK_IDX(h, PS_STRIDE, "holding"); };
    // a decision node's children (every lane of the wave asks together: the answer is wave-uniform); the slots past nact: node 0, never used
    auto kids = [&](uint32_t node, uint32_t nact, uint32_t (&ch)[4]) {
#pragma unroll
        for (int a = 0; a < 4; ++a) ch[a] = (uint32_t)a < nact ? uniform((uint32_t)tr.child[PK_IDX(node, RS_MAX_NODES, "child")][a]) : 0u;
    };

    for (uint32_t spot = blockIdx.x; spot < m; spot += gridDim.x) {
        __syncthreads();                              // (the spot before: its tree and its LDS arrays are done with)
        const uint32_t k = trees.tree_of ? uniform(trees.tree_of[spot]) : 0u;
        const bool good = k < ntrees;
        if (tid == 0 && out.status) out.status[spot] = good ? (uint8_t)0 : (uint8_t)PK_EQ_BAD_TREE;
        if (!solve) continue;
        // ---- the spot's tree into LDS (a refused spot: tree 0, which always exists, and none of it is used), and the slice laid out for it
        {
            const RsTree *src = trees.trees + (good ? PK_IDX(k, RS_MAX_TREES, "tree_of") : 0u);
            for (uint32_t w = tid; w < (uint32_t)(sizeof(RsTree) / 4); w += PS_BLOCK)
                reinterpret_cast<uint32_t *>(&tr)[PK_IDX(w, sizeof(RsTree) / 4, "tree")] = reinterpret_cast<const uint32_t *>(src)[w];
            __syncthreads();
            n = uniform(tr.n); pot = uniform(tr.pot);
            uint32_t dec = 0;
            for (uint32_t v = 0; v < n; ++v) dec += tr.kind[PK_IDX(v, RS_MAX_NODES, "kind")] <= RS_P1 ? 1u : 0u;
            D = good ? uniform(dec) : 0u;
            char *const base = ws + (size_t)blockIdx.x * ps_group_bytes(trees.nmax);
            const size_t plane = (size_t)n * PS_STRIDE;
            R = reinterpret_cast<int64_t *>(base); A = R + plane; U0 = A + plane; U1 = U0 + plane;
            RR = reinterpret_cast<uint64_t *>(U1 + plane);
            SG = reinterpret_cast<uint32_t *>(RR + plane);
        }
        const uint32_t DS = trees.Dmax;               // the row stride of `strategy`
        // ---- zeros: a refused spot's outputs, and the rows of `strategy` past the spot's own
        for (uint32_t h = tid; h < (uint32_t)RS_HOLDINGS; h += PS_BLOCK) {
            if (!good)
                for (uint32_t p = 0; p < 2u; ++p) {
                    if (out.value) out.value[((size_t)spot * 2 + p) * RS_HOLDINGS + h] = 0;
                    if (out.br) out.br[((size_t)spot * 2 + p) * RS_HOLDINGS + h] = 0;
                }
            if (out.strategy)
                for (uint32_t r = D * 4u; r < DS * 4u; ++r) out.strategy[((size_t)spot * DS * 4 + r) * RS_HOLDINGS + h] = 0;
        }
        if (!good) continue;
        // ---- the root's reaches; regrets and accumulators start at 0
        const uint16_t *w0 = ranges + (size_t)spot * 2 * RS_HOLDINGS, *w1 = w0 + RS_HOLDINGS;
#pragma unroll
        for (int j = 0; j < PS_PER_LANE; ++j) {
            const uint32_t h = tid + (uint32_t)j * PS_BLOCK;
            if (h >= (uint32_t)RS_HOLDINGS) continue;
            RR[at(0, h)] = ((uint64_t)w0[h] << 4) | ((uint64_t)w1[h] << 36);
            for (uint32_t v = 1; v < n; ++v) { R[at(v, h)] = 0; A[at(v, h)] = 0; }
        }

        // A terminal node: both players' values of every holding from the opponent's reaches (every lane of the workgroup comes here)
        auto terminal = [&](uint32_t node, uint32_t kind) {
#pragma unroll
            for (int j = 0; j < PS_PER_LANE; ++j) {
                const uint32_t h = tid + (uint32_t)j * PS_BLOCK;
                if (h < (uint32_t)RS_HOLDINGS) rq[PK_IDX(h, PS_STRIDE, "rq")] = RR[at(node, h)];
            }
            __syncthreads();
            // per-card sums: card x's 51 holdings
            if (tid < 52u) {
                uint64_t sum = 0;
                const uint32_t tt = tri(tid);
                for (uint32_t x = 0; x < 52u; ++x) sum += x == tid ? 0ull : rq[PK_IDX(pair(tid, tt, x, tri(x)), PS_STRIDE, "rq")];
                cs[PK_IDX(tid, 64, "cs")] = sum;
            }
            // the showdown's mat-vec: a wave per row of the table, the row's words coalesced across the lanes
            if (kind == RS_SHOWDOWN) {
                for (uint32_t row = wave; row < (uint32_t)RS_HOLDINGS; row += PS_WAVES) {
                    const uint32_t *wr = M + (size_t)row * PFM_HOLDINGS, *tr_ = wr + PFM_CELLS;
                    uint64_t a0 = 0, a1 = 0;
                    for (uint32_t c = lane; c < (uint32_t)RS_HOLDINGS; c += 64u) {
                        const uint32_t g = 2u * wr[c] + tr_[c];
                        const uint64_t r = rq[PK_IDX(c, PS_STRIDE, "rq")];
                        a0 += (uint64_t)(uint32_t)(r >> 32) * g;       // player 0 meets player 1's reach (the high halves)
                        a1 += (uint64_t)(uint32_t)r * g;
                    }
                    a0 = wave_sum(a0); a1 = wave_sum(a1);
                    if (lane == 0u) { E0[PK_IDX(row, PS_STRIDE, "E0")] = a0; E1[PK_IDX(row, PS_STRIDE, "E1")] = a1; }
                }
            }
            __syncthreads();
            uint64_t twice = 0;
            for (uint32_t x = 0; x < 52u; ++x) twice += cs[PK_IDX(x, 64, "cs")];
            const uint64_t all = ((uint64_t)((uint32_t)twice >> 1)) | ((twice >> 33) << 32);       // (each half is even)
            const uint32_t f = kind - RS_FOLD0, pf = tr.put[PK_IDX(node, RS_MAX_NODES, "put")][f & 1u], c = tr.put[PK_IDX(node, RS_MAX_NODES, "put")][0];
#pragma unroll
            for (int j = 0; j < PS_PER_LANE; ++j) {
                const uint32_t h = tid + (uint32_t)j * PS_BLOCK;
                if (h >= (uint32_t)RS_HOLDINGS) continue;
                // (no half borrows from the other: a holding's own entry is in both of its cards' sums, and the total holds them all)
                const uint64_t S = all - cs[PK_IDX(ha[j], 64, "cs")] - cs[PK_IDX(hb[j], 64, "cs")] + rq[PK_IDX(h, PS_STRIDE, "rq")];
                int64_t u0, u1;                       // player 0 meets player 1's reach (the high halves), player 1 the low ones
                if (kind == RS_SHOWDOWN) {
                    u0 = ps_share(E0[PK_IDX(h, PS_STRIDE, "E0")], pot + 2u * c) - (int64_t)(2u * c) * (int64_t)(S >> 32);
                    u1 = ps_share(E1[PK_IDX(h, PS_STRIDE, "E1")], pot + 2u * c) - (int64_t)(2u * c) * (int64_t)(uint32_t)S;
                } else {
                    const int64_t lose = -(int64_t)(2u * pf), gain = (int64_t)(2u * (pot + pf));
                    u0 = (f == 0u ? lose : gain) * (int64_t)(S >> 32);
                    u1 = (f == 1u ? lose : gain) * (int64_t)(uint32_t)S;
                }
                U0[at(node, h)] = u0;
                U1[at(node, h)] = u1;
            }
            __syncthreads();                          // (rq, cs and the sums are rewritten by the next terminal)
        };

        // One walk down: reaches, and every terminal's values.  from_r: the probabilities come from the regrets and are kept in SG;
        // otherwise SG is played as it stands.
        auto down = [&](bool from_r) {
            for (uint32_t node = 0; node < n; ++node) {
                const uint32_t kind = uniform((uint32_t)tr.kind[PK_IDX(node, RS_MAX_NODES, "kind")]);
                if (kind > RS_P1) { terminal(node, kind); continue; }
                const uint32_t nact = uniform((uint32_t)tr.nact[PK_IDX(node, RS_MAX_NODES, "nact")]);
                uint32_t ch[4];
                kids(node, nact, ch);
#pragma unroll
                for (int j = 0; j < PS_PER_LANE; ++j) {
                    const uint32_t h = tid + (uint32_t)j * PS_BLOCK;
                    if (h >= (uint32_t)RS_HOLDINGS) continue;
                    uint32_t sig[4];
                    if (from_r) {
                        int64_t X[4];
#pragma unroll
                        for (int a = 0; a < 4; ++a) X[a] = (uint32_t)a < nact ? R[at(ch[a], h)] : 0;
                        rs_sigma(X, nact, sig);
                    }
                    const uint64_t rr = RR[at(node, h)];
                    const uint32_t r0 = (uint32_t)rr, r1 = (uint32_t)(rr >> 32);
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        if ((uint32_t)a >= nact) continue;
                        const size_t e = at(ch[a], h);
                        if (from_r) SG[e] = sig[a]; else sig[a] = SG[e];
                        const uint32_t mine = (uint32_t)(((uint64_t)(kind == RS_P0 ? r0 : r1) * sig[a]) >> 15);
                        RR[e] = kind == RS_P0 ? ((uint64_t)mine | ((uint64_t)r1 << 32)) : ((uint64_t)r0 | ((uint64_t)mine << 32));
                    }
                }
            }
        };

        // ---- the iterations: one walk down, then the walk up with the regret and accumulator updates of each decision node
        for (uint32_t t = 1; t <= iters; ++t) {
            down(true);
            for (uint32_t node = n; node-- > 0u;) {
                const uint32_t kind = uniform((uint32_t)tr.kind[PK_IDX(node, RS_MAX_NODES, "kind")]);
                if (kind > RS_P1) continue;
                const uint32_t nact = uniform((uint32_t)tr.nact[PK_IDX(node, RS_MAX_NODES, "nact")]);
                int64_t *const Up = kind == RS_P0 ? U0 : U1, *const Uq = kind == RS_P0 ? U1 : U0;
                uint32_t ch[4];
                kids(node, nact, ch);
#pragma unroll
                for (int j = 0; j < PS_PER_LANE; ++j) {
                    const uint32_t h = tid + (uint32_t)j * PS_BLOCK;
                    if (h >= (uint32_t)RS_HOLDINGS) continue;
                    int64_t up[4], acc = 0, uq = 0;
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        up[a] = 0;
                        if ((uint32_t)a >= nact) continue;
                        const size_t e = at(ch[a], h);
                        up[a] = Up[e];
                        acc += (int64_t)SG[e] * up[a];
                        uq += Uq[e];
                    }
                    const int64_t un = acc >> 15;     // (the sum first, the floor once)
                    Up[at(node, h)] = un;
                    Uq[at(node, h)] = uq;
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        if ((uint32_t)a >= nact) continue;
                        const size_t e = at(ch[a], h);
                        const int64_t r = R[e] + up[a] - un;
                        R[e] = r > 0 ? r : 0;
                        const uint64_t rr = RR[e];
                        A[e] += (int64_t)((uint64_t)t * (uint64_t)(kind == RS_P0 ? (uint32_t)rr : (uint32_t)(rr >> 32)));
                    }
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
            for (int j = 0; j < PS_PER_LANE; ++j) {
                const uint32_t h = tid + (uint32_t)j * PS_BLOCK;
                if (h >= (uint32_t)RS_HOLDINGS) continue;
                int64_t X[4];
                uint32_t sig[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) X[a] = (uint32_t)a < nact ? A[at(ch[a], h)] : 0;
                rs_sigma(X, nact, sig);
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    if ((uint32_t)a < nact) SG[at(ch[a], h)] = sig[a];
                    if (out.strategy) out.strategy[(((size_t)spot * DS + PK_IDX(row, DS, "row")) * 4 + (uint32_t)a) * RS_HOLDINGS + h] = (uint16_t)sig[a];
                }
            }
        }
        if (!(out.value || out.br)) continue;
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
            for (int j = 0; j < PS_PER_LANE; ++j) {
                const uint32_t h = tid + (uint32_t)j * PS_BLOCK;
                if (h >= (uint32_t)RS_HOLDINGS) continue;
                int64_t acc = 0, uq = 0, bp = 0, bq = 0;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    if ((uint32_t)a >= nact) continue;
                    const size_t e = at(ch[a], h);
                    const int64_t up = Up[e], uqa = Uq[e], bpa = leaf[a] ? up : Bp[e], bqa = leaf[a] ? uqa : Bq[e];
                    acc += (int64_t)SG[e] * up;
                    uq += uqa;
                    bp = (a == 0 || bpa > bp) ? bpa : bp;
                    bq += bqa;
                }
                Up[at(node, h)] = acc >> 15;
                Uq[at(node, h)] = uq;
                Bp[at(node, h)] = bp;
                Bq[at(node, h)] = bq;
            }
        }
#pragma unroll
        for (int j = 0; j < PS_PER_LANE; ++j) {
            const uint32_t h = tid + (uint32_t)j * PS_BLOCK;
            if (h >= (uint32_t)RS_HOLDINGS) continue;
            const size_t o = (size_t)spot * 2 * RS_HOLDINGS + h;
            if (out.value) { out.value[o] = U0[at(0, h)]; out.value[o + RS_HOLDINGS] = U1[at(0, h)]; }
            if (out.br) { out.br[o] = R[at(0, h)]; out.br[o + RS_HOLDINGS] = A[at(0, h)]; }
        }
    }
}

namespace pk {

hipError_t ps_launch(hipStream_t stream, const uint32_t *M, const uint16_t *ranges, const RsTrees &trees, uint32_t ntrees, uint32_t iters, size_t m,
                     const RsOut &out, char *work) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_preflop_solve, dim3(ps_grid(m)), dim3(PS_BLOCK), 0, stream, M, ranges, trees, ntrees, out, work, iters, (uint32_t)m);
    return hipGetLastError();
}

}  // namespace pk
