// pk_equity_rvr.hip -- range against range: for EVERY holding the hero can have on a public board, the weight of the opponent's range it
// beats, ties and meets (include/pokerl_hip.h "Range vs range").  Row h of a spot is the agg[3] pk_equity_range gives
// for hero = h; here each seven-card hand is ranked once per completion of the board instead of once per hero.  Post-flop only.  Two kernels:
//   k_rvr_prep   one lane per spot: reads the spot (explicit arrays, or a handle's own tables: the board so far, no hole card), checks it,
//                writes its descriptor (known board, the pool mask, k = 5 - nb, P, boards) and its `boards` / `status`;
//   k_rvr        a persistent grid of 512-thread workgroups, each with the 32 KB rank-mask table of eval7_tab in LDS (staged once per
//                workgroup), ONE SPOT PER WORKGROUP at a time, spots dealt round robin.  Holdings are indexed by POOL SLOTS inside a spot
//                (ph = pb (pb - 1) / 2 + pa over the P <= 49 pool cards in canonical order, at most 1 176), so nothing is renumbered from one
//                completion to the next.  Per completion of the board (C(P, k) of them, the same for every lane):
//                  rank      every pool holding that shares no card with the completion is evaluated ONCE on board | completion | holding;
//                            its order key (larger = stronger, equal = tie: section 3.4) goes to keyw[ph] and, with ph below it, into a
//                            64-bit sort slot.  A holding that does share a card gets the sentinel, which sorts last and matches nothing;
//                  order     workgroup bitonic sort of the slots; an exclusive prefix sum of the weights in sorted order;
//                  combine   a lane finds, for each holding h it owns, the first sorted position of h's key and the first past it (binary
//                            search): the prefix sums there give the weight below and equal; the 2 (P - 2) holdings that share a card with h,
//                            and h itself, are taken back out by their own keys; what is left goes to h's 64-bit accumulators IN REGISTERS.
//                After the completions each lane writes win / tie / tot of h = tid, tid + 512, tid + 1024: all 1 326, coalesced, zeros included.
// Ordinary vector stores and LDS loads / stores only; no atomics, no scratch memory (tests/test_rvr_host.py reads the code objects).
#include <hip/hip_runtime.h>

#include "pk_equity_common.hpp"
#include "pk_equity_rvr.hpp"

using namespace pk;

#define RVR_PREP_BLOCK 256

struct RvrPrepArgs {
    RvrSpots s;
    EqTables t;
    RvrOut out;
    uint64_t *desc;
    size_t m;
};


template <bool TABLE>
__global__ void __launch_bounds__(RVR_PREP_BLOCK) k_rvr_prep(RvrPrepArgs a) {
    const size_t i = (size_t)blockIdx.x * RVR_PREP_BLOCK + threadIdx.x;
    if (i >= a.m) return;
    uint64_t *d = a.desc + i * (size_t)RVR_DESC_WORDS;
    uint32_t status = 0;
    int nb = 0;
    bool counted = true;               // nb is 0 .. 5: the pool can be measured against the cards the spot needs
    uint64_t dead = 0, known = 0;
    // one card byte: its bit in the suit-lane layout; marks it dead; a byte that is no card (0xFF too), or a card seen before, is refused
    auto card = [&](uint32_t c) -> uint64_t {
        if (c >= 0x40u || (c & 15u) >= 13u) { status |= PK_EQ_BAD_CARD; return 0; }
        const uint64_t bit = 1ull << ((c & 15u) * 4u + (c >> 4));              // canonical index (cards.py:77)
        status |= (dead & bit) ? (uint32_t)PK_EQ_DUP_CARD : 0u;
        dead |= bit;
        return 4ull << c;
    };
    if constexpr (TABLE) {
        const int64_t t = a.t.tables ? (int64_t)a.t.tables[i] : (int64_t)i;
        if (t < 0 || t >= (int64_t)a.t.T) { status |= PK_EQ_BAD_TABLE; counted = false; }   // (nothing is read)
        else {
            const Cursor cur{a.t.cursors[t]};
            if (cur.in_flight()) status |= PK_EQ_IN_FLIGHT;
            const int turn = (int)cur.turn();
            nb = turn == 0 ? 0 : (turn + 2 < 5 ? turn + 2 : 5);                 // game.py:266-278
            if (nb < 3) status |= PK_EQ_PREFLOP;
            for (int j = 0; j < nb; ++j) known |= card(card_byte(a.t.cards, (size_t)a.t.T, (int)t, j));   // (no hole card is read: the public board only)
        }
    } else {
        const uint32_t nbv = a.s.nboard[i];
        if (nbv > 5u) { status |= PK_EQ_BAD_NBOARD; counted = false; }
        else { nb = (int)nbv; if (nb < 3) status |= PK_EQ_PREFLOP; }
        for (int j = 0; j < nb; ++j) known |= card(a.s.board[i * 5 + j]);
        const uint64_t out_of_play = a.s.dead ? a.s.dead[i] : 0ull;
        if (out_of_play >> 52) status |= PK_EQ_BAD_CARD;
        const uint64_t dd = out_of_play & 0x000FFFFFFFFFFFFFull;
        if (dd & dead) status |= PK_EQ_DUP_CARD;
        dead |= dd;
    }
    const uint32_t P = 52u - (uint32_t)__popcll(dead), k = (uint32_t)(5 - nb);
    if (counted && P < k + 4u) status |= PK_EQ_SMALL_POOL;                      // the board to come and TWO holdings
    const uint32_t boards = status ? 0u : binom2(P - 4u, k);
    d[0] = known;
    d[1] = ~dead & 0x000FFFFFFFFFFFFFull;
    d[2] = (uint64_t)boards | ((uint64_t)k << 48) | ((uint64_t)P << 56);
    if (a.out.boards) a.out.boards[i] = boards;
    if (a.out.status) a.out.status[i] = (uint8_t)status;
}


// registers per lane: four waves per SIMD (two 512-thread workgroups per CU, what the group segment allows) cap a lane at 128 registers
__global__ void __launch_bounds__(RVR_BLOCK, 4) k_rvr(const uint32_t *__restrict__ tab, const uint64_t *__restrict__ desc, RvrWeights wts, RvrOut out,
                                                      uint32_t m) {
    __shared__ uint32_t T[EVAL7_TAB_WORDS];
    __shared__ uint64_t slot[RVR_SLOTS];              // key << 11 | pool holding, sorted per completion; all ones = no holding
    __shared__ uint32_t pre[RVR_PREFIX];              // pre[i]: the weight of sorted positions 0 .. i - 1
    __shared__ uint32_t keyw[RVR_POOL_HOLDINGS];      // this completion's key per pool holding (RVR_SENT: shares a card with the completion)
    __shared__ uint16_t wp[RVR_POOL_HOLDINGS];        // the spot's weights per pool holding
    __shared__ uint64_t pool[64];                     // card j of the pool (canonical order) as its bit in the suit-lane layout
    __shared__ uint32_t canon[64];                    // ... and its canonical index
    __shared__ uint32_t wsum[RVR_WAVES];
    stage_eval7_tab<RVR_BLOCK>(T, tab);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = uniform(tid >> 6);
    for (uint32_t spot = blockIdx.x; spot < m; spot += gridDim.x) {
        __syncthreads();                              // (the table; the spot before: its pool, weights, keys and sums are done with)
        const uint64_t *d = desc + (size_t)spot * RVR_DESC_WORDS;
        const uint64_t known = uniform(d[0]), avail = uniform(d[1]), meta = uniform(d[2]);
        const uint32_t boards = (uint32_t)meta, k = (uint32_t)(meta >> 48) & 0xffu, P = (uint32_t)(meta >> 56);
        uint64_t win[RVR_PER_LANE], tie[RVR_PER_LANE], tot[RVR_PER_LANE];
#pragma unroll
        for (int j = 0; j < RVR_PER_LANE; ++j) { win[j] = 0; tie[j] = 0; tot[j] = 0; }
        if (boards) {                                 // (a refused spot: zeros)
            fill_pool(pool, canon, avail, tid);
            __syncthreads();
            const uint32_t nh = tri(P), nreal = tri(P - k);   // pool holdings; those a completion leaves in play
            uint32_t npad = 64;
            while (npad < nh) npad <<= 1;                             // (> nh: C(P, 2) is no power of two for P >= 3, so a pad slot always exists)
            // ---- per spot: the pool holdings this lane ranks (ea < eb pool slots), the weights by pool holding, the pad slots
            const uint16_t *wv = wts.w ? wts.w + (wts.per_spot ? (size_t)spot * RVR_HOLDINGS : 0) : nullptr;
            uint64_t ebits[RVR_PER_LANE];
            uint32_t ea[RVR_PER_LANE], eb[RVR_PER_LANE], wmine = 0;
#pragma unroll
            for (int j = 0; j < RVR_PER_LANE; ++j) {
                const uint32_t ph = tid + (uint32_t)j * RVR_BLOCK;
                ea[j] = RVR_NONE; eb[j] = RVR_NONE; ebits[j] = 0;
                if (ph < nh) {
                    unpair(ph, ea[j], eb[j]);
                    ebits[j] = pool[PK_IDX(ea[j], 64, "pool")] | pool[PK_IDX(eb[j], 64, "pool")];
                    const uint32_t gh = tri(canon[PK_IDX(eb[j], 64, "canon")]) + canon[PK_IDX(ea[j], 64, "canon")];
                    const uint32_t w = wv ? (uint32_t)wv[PK_IDX(gh, RVR_HOLDINGS, "weights")] : 1u;
                    wp[PK_IDX(ph, RVR_POOL_HOLDINGS, "wp")] = (uint16_t)w;
                    wmine += w;
                }
            }
            for (uint32_t i = nh + tid; i < npad; i += RVR_BLOCK) slot[PK_IDX(i, RVR_SLOTS, "slot")] = ~0ull;   // (stay all ones: every sorted position >= nreal is)
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) wmine += __shfl_xor(wmine, off);
            if (lane == 0) wsum[PK_IDX(wave, RVR_WAVES, "wsum")] = wmine;
            // ... the holdings this lane OWNS (h = tid + 512 j of the fixed index space) as pool slots ha < hb; hph: their pool holding
            uint32_t ha[RVR_PER_LANE], hb[RVR_PER_LANE], hph[RVR_PER_LANE];
            bool hvalid[RVR_PER_LANE];
#pragma unroll
            for (int j = 0; j < RVR_PER_LANE; ++j) {
                const uint32_t h = tid + (uint32_t)j * RVR_BLOCK;
                uint32_t ca = 0, cb = 1;
                if (h < (uint32_t)RVR_HOLDINGS) unpair(h, ca, cb);
                hvalid[j] = h < (uint32_t)RVR_HOLDINGS && ((avail >> ca) & (avail >> cb) & 1ull);
                ha[j] = (uint32_t)__popcll(avail & ((1ull << ca) - 1ull));
                hb[j] = (uint32_t)__popcll(avail & ((1ull << cb) - 1ull));
                hph[j] = hvalid[j] ? tri(hb[j]) + ha[j] : 0u;
            }
            __syncthreads();
            uint32_t wall = 0;
#pragma unroll
            for (int w = 0; w < RVR_WAVES; ++w) wall += wsum[PK_IDX(w, RVR_WAVES, "wsum")];
            // tot[h] = boards * (the weight of the valid holdings that share no card with h)
#pragma unroll
            for (int j = 0; j < RVR_PER_LANE; ++j) {
                if (!hvalid[j]) continue;
                uint32_t conf = wp[PK_IDX(hph[j], RVR_POOL_HOLDINGS, "wp")];
                const uint32_t ta = tri(ha[j]), tb = tri(hb[j]);
                for (uint32_t x = 0; x < P; ++x) {
                    if (x == ha[j] || x == hb[j]) continue;
                    const uint32_t tx = tri(x);
                    conf += (uint32_t)wp[PK_IDX(pair(ha[j], ta, x, tx), RVR_POOL_HOLDINGS, "wp")] +
                            (uint32_t)wp[PK_IDX(pair(hb[j], tb, x, tx), RVR_POOL_HOLDINGS, "wp")];
                }
                tot[j] = (uint64_t)boards * (uint64_t)(wall - conf);
            }
            // ---- the completions: {ci < cj} in pair order (k = 2), {c} (k = 1), {} (k = 0)
            const uint32_t ncomp = binom2(P, k);
            uint32_t ci = 0, cj = 1;
            for (uint32_t c = 0; c < ncomp; ++c) {
                const uint32_t x0 = k == 2u ? ci : (k == 1u ? c : RVR_NONE), x1 = k == 2u ? cj : RVR_NONE;
                const uint64_t board = known | pool[PK_IDX(x0, 64, "pool")] | pool[PK_IDX(x1, 64, "pool")];
                // rank
#pragma unroll
                for (int j = 0; j < RVR_PER_LANE; ++j) {
                    const uint32_t ph = tid + (uint32_t)j * RVR_BLOCK;
                    if (ph < nh) {
                        const bool gone = ea[j] == x0 || ea[j] == x1 || eb[j] == x0 || eb[j] == x1;
                        uint32_t key = RVR_SENT;
                        if (!gone) key = order_key(eval7_tab_back(eval7_tab_front_bits(board | ebits[j], T), T));
                        keyw[PK_IDX(ph, RVR_POOL_HOLDINGS, "keyw")] = key;
                        slot[PK_IDX(ph, RVR_SLOTS, "slot")] = gone ? ~0ull : (((uint64_t)key << 11) | ph);
                    }
                }
                __syncthreads();
                // order: bitonic sort of slot[0 .. npad), ascending
                for (uint32_t kk = 2; kk <= npad; kk <<= 1) {
                    for (uint32_t jj = kk >> 1; jj > 0; jj >>= 1) {
                        for (uint32_t t = tid; t < (npad >> 1); t += RVR_BLOCK) {
                            const uint32_t lo = ((t & ~(jj - 1u)) << 1) | (t & (jj - 1u)), hi = lo | jj;
                            const uint64_t a = slot[PK_IDX(lo, RVR_SLOTS, "slot")], b = slot[PK_IDX(hi, RVR_SLOTS, "slot")];
                            const bool up = (lo & kk) == 0u;
                            if ((a > b) == up) { slot[PK_IDX(lo, RVR_SLOTS, "slot")] = b; slot[PK_IDX(hi, RVR_SLOTS, "slot")] = a; }
                        }
                        __syncthreads();
                    }
                }
                // exclusive prefix sum of the weights in sorted order: three positions per lane, a wave scan, the waves' totals
                uint32_t v[RVR_PER_LANE], mine = 0;
#pragma unroll
                for (int j = 0; j < RVR_PER_LANE; ++j) {
                    const uint32_t i = tid * RVR_PER_LANE + (uint32_t)j;
                    v[j] = 0;
                    if (i < nreal) v[j] = wp[PK_IDX((uint32_t)slot[PK_IDX(i, RVR_SLOTS, "slot")] & 2047u, RVR_POOL_HOLDINGS, "wp")];
                    mine += v[j];
                }
                uint32_t inc = mine;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t y = __shfl_up(inc, off);
                    inc += lane >= (uint32_t)off ? y : 0u;
                }
                if (lane == 63u) wsum[PK_IDX(wave, RVR_WAVES, "wsum")] = inc;
                __syncthreads();
                uint32_t run = inc - mine;
#pragma unroll
                for (int w = 0; w < RVR_WAVES; ++w) run += (uint32_t)w < wave ? wsum[PK_IDX(w, RVR_WAVES, "wsum")] : 0u;
#pragma unroll
                for (int j = 0; j < RVR_PER_LANE; ++j) {
                    pre[PK_IDX(tid * RVR_PER_LANE + (uint32_t)j, RVR_PREFIX, "pre")] = run;
                    run += v[j];
                }
                __syncthreads();
                // combine
#pragma unroll
                for (int j = 0; j < RVR_PER_LANE; ++j) {
                    if (!hvalid[j]) continue;
                    const uint32_t kh = keyw[PK_IDX(hph[j], RVR_POOL_HOLDINGS, "keyw")];
                    if (kh == RVR_SENT) continue;                                   // (h shares a card with this completion)
                    uint32_t lb = 0, ub = 0;                                        // sorted positions with a key < kh, <= kh
                    for (uint32_t step = npad >> 1; step > 0; step >>= 1) {
                        const uint32_t kl = (uint32_t)(slot[PK_IDX(lb + step - 1u, RVR_SLOTS, "slot")] >> 11);
                        const uint32_t ku = (uint32_t)(slot[PK_IDX(ub + step - 1u, RVR_SLOTS, "slot")] >> 11);
                        lb += kl < kh ? step : 0u;
                        ub += ku <= kh ? step : 0u;
                    }
                    const uint32_t below0 = pre[PK_IDX(lb, RVR_PREFIX, "pre")];
                    uint32_t below = below0, equal = pre[PK_IDX(ub, RVR_PREFIX, "pre")] - below0;
                    // card removal: h itself, and every holding {ha, x}, {hb, x}
                    equal -= wp[PK_IDX(hph[j], RVR_POOL_HOLDINGS, "wp")];
                    const uint32_t ta = tri(ha[j]), tb = tri(hb[j]);
                    for (uint32_t x = 0; x < P; ++x) {
                        if (x == ha[j] || x == hb[j]) continue;
                        const uint32_t tx = tri(x);
                        const uint32_t p0 = PK_IDX(pair(ha[j], ta, x, tx), RVR_POOL_HOLDINGS, "pair"), p1 = PK_IDX(pair(hb[j], tb, x, tx), RVR_POOL_HOLDINGS, "pair");
                        const uint32_t k0 = keyw[p0], k1 = keyw[p1], w0 = wp[p0], w1 = wp[p1];   // (p0, p1: checked above)
                        below -= (k0 < kh ? w0 : 0u) + (k1 < kh ? w1 : 0u);
                        equal -= (k0 == kh ? w0 : 0u) + (k1 == kh ? w1 : 0u);
                    }
                    win[j] += below;
                    tie[j] += equal;
                }
                __syncthreads();                      // (the keys and slots are rewritten by the next completion)
                ++ci;
                if (ci == cj) { ci = 0; ++cj; }
            }
        }
        // ---- output: every holding's sums (zeros included)
#pragma unroll
        for (int j = 0; j < RVR_PER_LANE; ++j) {
            const uint32_t h = tid + (uint32_t)j * RVR_BLOCK;
            if (h < (uint32_t)RVR_HOLDINGS) {
                if (out.win) out.win[(size_t)spot * RVR_HOLDINGS + h] = win[j];
                if (out.tie) out.tie[(size_t)spot * RVR_HOLDINGS + h] = tie[j];
                if (out.tot) out.tot[(size_t)spot * RVR_HOLDINGS + h] = tot[j];
            }
        }
    }
}

namespace pk {

hipError_t rvr_prep_launch(hipStream_t stream, const RvrSpots *spots, const EqTables *tables, size_t m, const RvrOut &out, uint64_t *desc) {
    RvrPrepArgs a{};
    if (spots) a.s = *spots;
    if (tables) a.t = *tables;
    a.out = out; a.desc = desc; a.m = m;
    const dim3 pgrid((unsigned)((m + RVR_PREP_BLOCK - 1) / RVR_PREP_BLOCK));
    if (tables) hipLaunchKernelGGL(k_rvr_prep<true>, pgrid, dim3(RVR_PREP_BLOCK), 0, stream, a);
    else hipLaunchKernelGGL(k_rvr_prep<false>, pgrid, dim3(RVR_PREP_BLOCK), 0, stream, a);
    return hipGetLastError();
}

hipError_t rvr_launch(hipStream_t stream, const uint32_t *tab, const RvrSpots *spots, const EqTables *tables, const RvrWeights &weights, size_t m,
                      const RvrOut &out, uint64_t *desc) {
    if (m == 0) return hipSuccess;
    const hipError_t e = rvr_prep_launch(stream, spots, tables, m, out, desc);
    if (e != hipSuccess || !(out.win || out.tie || out.tot)) return e;   // (boards / status alone: the preparation kernel has written them)
    // one workgroup per spot at a time (each stages the 32 KB table); the grid is persistent beyond two workgroups per CU
    const unsigned grid = (unsigned)(m < (size_t)RVR_GRID_MAX ? m : (size_t)RVR_GRID_MAX);
    hipLaunchKernelGGL(k_rvr, dim3(grid), dim3(RVR_BLOCK), 0, stream, tab, (const uint64_t *)desc, weights, out, (uint32_t)m);
    return hipGetLastError();
}

}  // namespace pk
