// pk_equity_range.hpp -- exact hand strength against ONE hidden hand (include/pokerl_hip.h "Range equity"): what the
// host entry points (pk_api.hip) and the kernels (pk_equity_range.hip) share.  The table kernels do not include it.
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

// Queues the whole call on `stream`: descriptors + boards / status (one lane per spot), then the persistent enumeration kernel.
// tab: the evaluator table (eval7_table); `tables` non-NULL selects the table form (observer: a seat or PK_OBSERVER_ACTIVE).
hipError_t eqr_launch(hipStream_t stream, const uint32_t *tab, const EqrSpots *spots, const EqTables *tables, int N, int observer,
                      const EqrWeights &weights, size_t m, const EqrOut &out, uint64_t *desc);
// The first half alone, for the hero histograms (pk_equity_hist_hero.hip), whose spot is this one: k_eqr_prep on `stream` -- the descriptors,
// and out.boards / out.status where they are given (the other outputs are not looked at).
hipError_t eqr_prep_launch(hipStream_t stream, const EqrSpots *spots, const EqTables *tables, int N, int observer, size_t m, const EqrOut &out,
                           uint64_t *desc);

}  // namespace pk
