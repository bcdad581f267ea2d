// pk_equity_range.hpp -- exact hand strength against ONE hidden hand (include/pokerl_hip.h "Range equity"): what the
// host entry points (pk_api.hip) and the kernels (pk_equity_range.hip) share, and the device passes k_eqr shares with k_hero_hist.  The
// table kernels do not include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pk_equity.hpp"

namespace pk {

constexpr int EQR_HOLDINGS = PK_EQ_HOLDINGS;            // C(52, 2) unordered pairs: h = b (b - 1) / 2 + a, canonical indices a < b
constexpr int EQR_BLOCK = 512, EQR_WAVES = EQR_BLOCK / 64;
constexpr int EQR_GRID_MAX = 768;                        // persistent grid: three 512-thread workgroups per CU (3 x ~48 KB of LDS)
constexpr int EQR_COMPLETIONS = 1081;                    // C(47, 2): board completions of a full-pool flop (the hero's words)
constexpr int EQR_DESC_WORDS = 4;
// A spot's descriptor: 4 64-bit words.
//   [0] known board cards, [1] the hero's two cards: suit-lane bit sets OR(4 << Card.value), what eval7_tab_front_bits takes
//   [2] the pool: bit c set = the card of canonical index c (rank0 * 4 + suit) is not dead
//   [3] boards | k << 48 | P << 56   (k = 5 - nb cards to come, P = cards in the pool; boards = 0 for a refused spot)
inline size_t eqr_work_bytes(size_t m) { return m * EQR_DESC_WORDS * sizeof(uint64_t); }

struct EqrSpots {         // the explicit form
    const uint8_t *hero, *board, *nboard;
    const uint64_t *dead;    // NULL: none
};
struct EqrOut {           // any may be NULL
    uint64_t *agg;
    uint32_t *win, *tie, *boards;
    uint8_t *status;
};
struct EqrWeights {
    const uint16_t *w;       // NULL: every weight is 1
    int per_spot;            // 0: one vector [1326] for the call, 1: [m][1326]
};

// ---- what the two kernels of this spot (k_eqr, and k_hero_hist of pk_equity_hist_hero.hip) share: a workgroup of EQR_BLOCK threads, the
// evaluator table T, the pool (pk::fill_pool) and the hero's words in LDS.
// The hero pass: the hero's ranking word on each of the ncomp = C(P, k) completions of the board, into hero_w at the completion's
// index -- {i < j} at j (j - 1) / 2 + i, {i} at i, {} at 0.  hand: known board | hero.  A barrier follows at the caller's.
__device__ __forceinline__ void eqr_hero_pass(const uint32_t *T, const uint64_t *pool, uint32_t *hero_w, uint64_t hand, uint32_t k, uint32_t ncomp,
                                              uint32_t tid) {
    for (uint32_t c = tid; c < ncomp; c += EQR_BLOCK) {
        uint64_t bits = hand;
        if (k == 2u) { uint32_t ci, cj; unpair(c, ci, cj); bits |= pool[PK_IDX(ci, 64, "pool") & 63u] | pool[PK_IDX(cj, 64, "pool") & 63u]; }
        else if (k == 1u) bits |= pool[PK_IDX(c, 64, "pool") & 63u];
        hero_w[PK_IDX(c, EQR_COMPLETIONS, "hero_w")] = eval7_tab_back(eval7_tab_front_bits(bits, T), T);
    }
}
// The villain pass: the villain's seven cards are the known board plus a set S of s = k + 2 pool cards, whichever way S splits into "board
// to come" and "hole cards".  Lanes enumerate the sets S in lexicographic order (a contiguous index range per lane, unranked once, then
// stepped: Comb<4, 2>, the first 2 - k levels frozen), evaluate board | S ONCE, and for each of the C(s, 2) splits look the hero's word of
// that completion up, decide with compare_rankings<2> and call count(completion, holding, win): the completion's index in hero_w, the
// hole cards' holding in the fixed 1 326 index space, win = 1 the hero wins, 3 a tie, 2 the villain wins.
template <typename F>
__device__ __forceinline__ void eqr_villain_pass(const uint32_t *T, const uint64_t *pool, const uint32_t *canon, const uint32_t *hero_w, uint64_t known,
                                                 uint32_t k, uint32_t P, uint32_t tid, F &&count) {
    const uint32_t s = k + 2u;
    const uint32_t nsets = s == 2u ? binom_c<2>(P) : (s == 3u ? binom_c<3>(P) : (uint32_t)((uint64_t)binom_c<3>(P) * (P - 3u) / 4u));
    const uint32_t per = (nsets + EQR_BLOCK - 1u) / EQR_BLOCK, s0 = tid * per;      // this lane's sets [s0, s0 + cnt)
    const uint32_t cnt = s0 < nsets ? min(per, nsets - s0) : 0u;
    const int f = 4 - (int)s;
    Comb<4, 2> cb;
    cb.start(P, f, s0, cnt != 0);
    uint64_t base = known | pool[PK_IDX(cb.c[0], 64, "pool") & 63u] | pool[PK_IDX(cb.c[1], 64, "pool") & 63u] | pool[PK_IDX(cb.c[2], 64, "pool") & 63u];
    uint32_t n0 = canon[PK_IDX(cb.c[0], 64, "canon") & 63u], n1 = canon[PK_IDX(cb.c[1], 64, "canon") & 63u], n2 = canon[PK_IDX(cb.c[2], 64, "canon") & 63u];
    for (uint32_t n = 0; n < cnt; ++n) {
        const uint32_t c0 = cb.c[0], c1 = cb.c[1], c2 = cb.c[2], j = cb.c[3];
        const uint32_t nj = canon[PK_IDX(j, 64, "canon") & 63u];
        const uint32_t vil = eval7_tab_back(eval7_tab_front_bits(base | pool[PK_IDX(j, 64, "pool") & 63u], T), T);
        // one split: levels x < y are the villain's hole cards (canonical nx < ny), levels u < v the board to come
        auto split = [&](int x, uint32_t nx, uint32_t ny, uint32_t lu, uint32_t lv) {
            if (x < f) return;                                                   // (uniform: a level that does not exist)
            const uint32_t comp = PK_IDX(k == 2u ? tri(lv) + lu : (k == 1u ? lv : 0u), EQR_COMPLETIONS, "completion");
            const uint32_t v[2] = {hero_w[comp], vil};
            int nw;
            const uint32_t win = compare_rankings<2>(v, nw);
            count(comp, PK_IDX(tri(ny) + nx, EQR_HOLDINGS, "holding"), win);
        };
        split(0, n0, n1, c2, j);
        split(0, n0, n2, c1, j);
        split(0, n0, nj, c1, c2);
        split(1, n1, n2, c0, j);
        split(1, n1, nj, c0, c2);
        split(2, n2, nj, c0, c1);
        cb.next(P, [&] {
            base = known | pool[PK_IDX(cb.c[0], 64, "pool") & 63u] | pool[PK_IDX(cb.c[1], 64, "pool") & 63u] | pool[PK_IDX(cb.c[2], 64, "pool") & 63u];
            n0 = canon[PK_IDX(cb.c[0], 64, "canon") & 63u]; n1 = canon[PK_IDX(cb.c[1], 64, "canon") & 63u]; n2 = canon[PK_IDX(cb.c[2], 64, "canon") & 63u];
        });
    }
}

// Queues the whole call on `stream`: descriptors + boards / status (one lane per spot), then the persistent enumeration kernel.
// tab: the evaluator table (eval7_table); `tables` non-NULL selects the table form (observer: a seat or PK_OBSERVER_ACTIVE).
hipError_t eqr_launch(hipStream_t stream, const uint32_t *tab, const EqrSpots *spots, const EqTables *tables, int N, int observer,
                      const EqrWeights &weights, size_t m, const EqrOut &out, uint64_t *desc);
// The first half alone, for the hero histograms (pk_equity_hist_hero.hip), whose spot is this one: k_eqr_prep on `stream` -- the descriptors,
// and out.boards / out.status where they are given (the other outputs are not looked at).
hipError_t eqr_prep_launch(hipStream_t stream, const EqrSpots *spots, const EqTables *tables, int N, int observer, size_t m, const EqrOut &out,
                           uint64_t *desc);

}  // namespace pk
