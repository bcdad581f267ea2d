// pk_equity_range.hip -- exact hand strength against ONE hidden hand: the hero's result against every holding the hidden opponent can
// have, per holding and reduced by a range of weights (include/pokerl_hip.h "Range equity").  Post-flop only
// (nb = 3, 4, 5): pre-flop a hidden hand is 2 * 10^9 boards per spot, and the pre-flop hero-versus-holding table is a constant nobody needs
// recomputed -- PK_EQ_PREFLOP.  Two kernels per call:
//   k_eqr_prep   one lane per spot: reads the spot (explicit arrays, or a handle's own tables as one seat sees them), checks it, writes its
//                descriptor (known board and hero as suit-lane bit sets, the pool mask, k = 5 - nb, P, boards) and its `boards` / `status`;
//   k_eqr        a persistent grid of 512-thread workgroups, each with the 32 KB rank-mask table of eval7_tab in LDS (staged once per
//                workgroup), ONE SPOT PER WORKGROUP at a time, spots dealt round robin.  Per spot:
//                  hero pass     the hero's ranking word on each of the C(P, k) completions of the board, into LDS at the completion's
//                                pair / single index;
//                  villain pass  the villain's seven cards are the known board plus a set S of k + 2 pool cards, whichever way S splits into
//                                "board to come" and "hole cards".  Lanes enumerate the sets S (a contiguous index range per lane, unranked
//                                once, then stepped), evaluate board | S ONCE, and for each of the C(k + 2, 2) splits look the hero's word of
//                                that completion up, decide with compare_rankings<2> and add to the LDS counters of that split's holding
//                                (two u32 per holding in the fixed 1 326 index space, LDS atomics).  One loop serves nb = 3, 4, 5;
//                                The two passes are functions of pk_equity_range.hpp, shared with k_hero_hist (pk_equity_hist_hero.hip);
//                  output        all 1 326 win / tie entries from LDS, coalesced, zeros included (no memset); the weighted sums reduced
//                                over the workgroup in 64 bits and written by one lane; the counters cleared for the next spot.
// Ordinary vector stores and LDS atomics only; no scratch memory (tests/test_equity_range_host.py reads the code objects).
#include <hip/hip_runtime.h>

#include "pk_equity_common.hpp"
#include "pk_equity_range.hpp"

using namespace pk;

#define EQR_PREP_BLOCK 256

struct EqrPrepArgs {
    EqrSpots s;
    EqTables t;
    EqrOut out;
    uint64_t *desc;
    int N, observer;
    size_t m;
};


template <bool TABLE>
__global__ void __launch_bounds__(EQR_PREP_BLOCK) k_eqr_prep(EqrPrepArgs a) {
    const size_t i = (size_t)blockIdx.x * EQR_PREP_BLOCK + threadIdx.x;
    if (i >= a.m) return;
    uint64_t *d = a.desc + i * (size_t)EQR_DESC_WORDS;
    uint32_t status = 0;
    int nb = 0;
    bool counted = true;               // nb is 0 .. 5: the pool can be measured against the cards the spot needs
    uint64_t dead = 0, known = 0, hero = 0;
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
            const int who = a.observer == PK_OBSERVER_ACTIVE ? (int)cur.active() : a.observer;
            if (who < 0 || who >= a.N) status |= PK_EQ_BAD_CARD;                // (a cursor no game writes: there is no such seat to read)
            else {
                hero = card(card_byte(a.t.cards, (size_t)a.t.T, (int)t, 5 + 2 * who));
                hero |= card(card_byte(a.t.cards, (size_t)a.t.T, (int)t, 6 + 2 * who));
            }
            for (int j = 0; j < nb; ++j) known |= card(card_byte(a.t.cards, (size_t)a.t.T, (int)t, j));   // (the later streets' cards the deck holds are in the pool)
        }
    } else {
        const uint32_t nbv = a.s.nboard[i];
        if (nbv > 5u) { status |= PK_EQ_BAD_NBOARD; counted = false; }
        else { nb = (int)nbv; if (nb < 3) status |= PK_EQ_PREFLOP; }
        hero = card(a.s.hero[i * 2]);
        hero |= card(a.s.hero[i * 2 + 1]);
        for (int j = 0; j < nb; ++j) known |= card(a.s.board[i * 5 + j]);
        const uint64_t out_of_play = a.s.dead ? a.s.dead[i] : 0ull;
        if (out_of_play >> 52) status |= PK_EQ_BAD_CARD;
        const uint64_t dd = out_of_play & 0x000FFFFFFFFFFFFFull;
        if (dd & dead) status |= PK_EQ_DUP_CARD;
        dead |= dd;
    }
    const uint32_t P = 52u - (uint32_t)__popcll(dead), k = (uint32_t)(5 - nb);
    if (counted && P < k + 2u) status |= PK_EQ_SMALL_POOL;
    const uint32_t boards = status ? 0u : binom2(P - 2u, k);
    d[0] = known;
    d[1] = hero;
    d[2] = ~dead & 0x000FFFFFFFFFFFFFull;
    d[3] = (uint64_t)boards | ((uint64_t)k << 48) | ((uint64_t)P << 56);
    if (a.out.boards) a.out.boards[i] = boards;
    if (a.out.status) a.out.status[i] = (uint8_t)status;
}


// registers per lane: six waves per SIMD (three 512-thread workgroups per CU, what the group segment allows) caps a lane at 80 registers; the kernel uses 72, no spill
__global__ void __launch_bounds__(EQR_BLOCK, 6) k_eqr(const uint32_t *__restrict__ tab, const uint64_t *__restrict__ desc, EqrWeights wts, EqrOut out,
                                                      uint32_t m) {
    __shared__ uint32_t T[EVAL7_TAB_WORDS];
    __shared__ uint64_t pool[64];                 // card j of the pool (canonical order) as its bit in the suit-lane layout
    __shared__ uint32_t canon[64];                // ... and its canonical index
    __shared__ uint32_t hero_w[EQR_COMPLETIONS];  // the hero's ranking word per completion of the board
    __shared__ uint32_t cwin[EQR_HOLDINGS], ctie[EQR_HOLDINGS];
    __shared__ uint64_t red[EQR_WAVES][3];
    stage_eval7_tab<EQR_BLOCK>(T, tab);
    for (int h = threadIdx.x; h < EQR_HOLDINGS; h += EQR_BLOCK) { cwin[PK_IDX(h, EQR_HOLDINGS, "cwin")] = 0; ctie[PK_IDX(h, EQR_HOLDINGS, "ctie")] = 0; }
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = uniform(tid >> 6);
    for (uint32_t spot = blockIdx.x; spot < m; spot += gridDim.x) {
        __syncthreads();                          // (the table and the cleared counters; the spot before: its pool, hero words and sums are done with)
        const uint64_t *d = desc + (size_t)spot * EQR_DESC_WORDS;
        const uint64_t known = uniform(d[0]), hero = uniform(d[1]), avail = uniform(d[2]), meta = uniform(d[3]);
        const uint32_t boards = (uint32_t)meta, k = (uint32_t)(meta >> 48) & 0xffu, P = (uint32_t)(meta >> 56);
        if (boards) {                             // (a refused spot: its counters stay zero)
            fill_pool(pool, canon, avail, tid);
            __syncthreads();
            eqr_hero_pass(T, pool, hero_w, known | hero, k, binom2(P, k), tid);
            __syncthreads();
            // the villain pass: a split counts for its holding
            eqr_villain_pass(T, pool, canon, hero_w, known, k, P, tid, [&](uint32_t, uint32_t h, uint32_t win) {
                if (win == 1u) atomicAdd(&cwin[h], 1u);
                else if (win == 3u) atomicAdd(&ctie[h], 1u);
            });
            __syncthreads();
        }
        // ---- output: every holding's counters (zeros included), the weighted sums, and the counters cleared for the next spot
        const uint16_t *wv = wts.w ? wts.w + (wts.per_spot ? (size_t)spot * EQR_HOLDINGS : 0) : nullptr;
        uint64_t a0 = 0, a1 = 0, a2 = 0;
        for (uint32_t h = tid; h < (uint32_t)EQR_HOLDINGS; h += EQR_BLOCK) {
            const uint32_t w = cwin[PK_IDX(h, EQR_HOLDINGS, "cwin")], t = ctie[PK_IDX(h, EQR_HOLDINGS, "ctie")];
            cwin[h] = 0; ctie[h] = 0;
            if (out.win) out.win[(size_t)spot * EQR_HOLDINGS + h] = w;
            if (out.tie) out.tie[(size_t)spot * EQR_HOLDINGS + h] = t;
            if (out.agg) {
                const uint64_t wt = wv ? (uint64_t)wv[h] : 1ull;
                uint32_t ca, cb;
                unpair(h, ca, cb);
                const bool valid = boards && ((avail >> ca) & (avail >> cb) & 1ull);
                a0 += wt * w; a1 += wt * t; a2 += valid ? wt : 0ull;
            }
        }
        if (out.agg) {
            a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
            if (lane == 0) { red[PK_IDX(wave, EQR_WAVES, "red")][0] = a0; red[wave][1] = a1; red[wave][2] = a2; }
            __syncthreads();
            if (tid == 0) {
                uint64_t r0 = 0, r1 = 0, r2 = 0;
                for (int wv_ = 0; wv_ < EQR_WAVES; ++wv_) { r0 += red[PK_IDX(wv_, EQR_WAVES, "red")][0]; r1 += red[wv_][1]; r2 += red[wv_][2]; }
                out.agg[(size_t)spot * 3] = r0;
                out.agg[(size_t)spot * 3 + 1] = r1;
                out.agg[(size_t)spot * 3 + 2] = (uint64_t)boards * r2;
            }
        }
    }
}

namespace pk {

hipError_t eqr_prep_launch(hipStream_t stream, const EqrSpots *spots, const EqTables *tables, int N, int observer, size_t m, const EqrOut &out,
                           uint64_t *desc) {
    EqrPrepArgs a{};
    if (spots) a.s = *spots;
    if (tables) a.t = *tables;
    a.out = out; a.desc = desc; a.N = N; a.observer = observer; a.m = m;
    const dim3 pgrid((unsigned)((m + EQR_PREP_BLOCK - 1) / EQR_PREP_BLOCK));
    if (tables) hipLaunchKernelGGL(k_eqr_prep<true>, pgrid, dim3(EQR_PREP_BLOCK), 0, stream, a);
    else hipLaunchKernelGGL(k_eqr_prep<false>, pgrid, dim3(EQR_PREP_BLOCK), 0, stream, a);
    return hipGetLastError();
}

hipError_t eqr_launch(hipStream_t stream, const uint32_t *tab, const EqrSpots *spots, const EqTables *tables, int N, int observer,
                      const EqrWeights &weights, size_t m, const EqrOut &out, uint64_t *desc) {
    if (m == 0) return hipSuccess;
    const hipError_t e = eqr_prep_launch(stream, spots, tables, N, observer, m, out, desc);
    if (e != hipSuccess || !(out.agg || out.win || out.tie)) return e;   // (boards / status alone: the preparation kernel has written them)
    // one workgroup per spot at a time (each stages the 32 KB table); the grid is persistent beyond three workgroups per CU
    const unsigned grid = (unsigned)(m < (size_t)EQR_GRID_MAX ? m : (size_t)EQR_GRID_MAX);
    hipLaunchKernelGGL(k_eqr, dim3(grid), dim3(EQR_BLOCK), 0, stream, tab, (const uint64_t *)desc, weights, out, (uint32_t)m);
    return hipGetLastError();
}

}  // namespace pk
