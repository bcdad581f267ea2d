// pk_equity_ranged.hpp -- sampled showdown equity against WEIGHTED RANGES: every hidden seat draws its holding from a u16 [1326] range
// (include/pokerl_hip.h "Ranged sampled equity"): what the host entry points (pk_api.hip) and the kernels
// (pk_equity_ranged.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pk_equity_sampled.hpp"

namespace pk {

constexpr uint32_t STREAM_EQW = 0x45515730u;            // 'EQW0' (+ block b = 0 .. 8): the ranged equity's own Philox stream
constexpr int EQW_HOLDINGS = PK_EQ_HOLDINGS;            // 1326, h = b (b - 1) / 2 + a over canonical indices a < b
constexpr int EQW_MAX_RANGES = PK_EQW_MAX_RANGES;       // rows of a call's weight table at most: they sit in LDS beside the evaluator table
constexpr uint32_t EQW_UNIFORM = PK_EQW_UNIFORM;        // range_of entry: every weight 1 (cum[h] = h + 1, no LDS row)
constexpr size_t EQW_ROW_BYTES = (size_t)EQW_HOLDINGS * 4;   // one row of cumulative sums: 5 304 B

// LDS size classes of k_eqw<N, RC>: RC rows of cumulative sums beside the 32 KB evaluator table and the 2.6 KB holding -> cards table.
//   RC = 0   R = 0 (every hidden seat uniform)   35.5 KB: four workgroups per CU, as k_eqs
//   RC = 8   R = 1 .. 8                          77.9 KB: two workgroups per CU
//   RC = 16  R = 9 .. 16                         120.4 KB: one workgroup per CU
constexpr int eqw_class(uint32_t R) { return R == 0 ? 0 : (R <= 8 ? 8 : 16); }
constexpr size_t eqw_lds_bytes(int RC) { return (size_t)EVAL7_TAB_WORDS * 4 + (size_t)RC * EQW_ROW_BYTES + (size_t)EQW_HOLDINGS * 2 + 128; }
static_assert(2 * eqw_lds_bytes(8) <= 160 * 1024 && eqw_lds_bytes(16) <= 160 * 1024 && 4 * eqw_lds_bytes(0) <= 160 * 1024, "the LDS of a CU");

// A spot's descriptor: 8 + N 64-bit words, written by k_eqw_prep.
//   [0] known board cards, [8 + p] seat p's KNOWN hole cards: suit-lane bit sets OR(4 << Card.value), what eval7_tab_front_bits takes
//   [1] the pool: bit c set = the card of canonical index c (rank0 * 4 + suit) is not dead
//   [2] hidden seats (bit p: live seat p draws its holding) | live << 32 | k << 48 | P << 56   (k = 5 - nb board cards to draw)
//   [3] stream id | valid << 32   (valid = 0: a refused spot, no attempts)
//   [4 + p / 4] bits 16 (p % 4) ..: seat p's range row, EQW_UNIFORM = the uniform row (written for every seat, read where it is hidden)
constexpr int eqw_desc_words(int N) { return 8 + N; }
// Work space of one call: the cumulative sums u32 [R][1326], then the descriptors.
inline size_t eqw_cum_bytes(uint32_t R) { return (size_t)R * EQW_ROW_BYTES; }
inline size_t eqw_work_bytes(int N, size_t m, uint32_t R) { return eqw_cum_bytes(R) + m * (size_t)eqw_desc_words(N) * 8; }

struct EqwOut {           // any may be NULL
    uint32_t *win, *tie;
    uint64_t *share;
    uint32_t *accepted;
    uint8_t *status;
};
struct EqwRanges {        // weights u16 [R][1326]; range_of u16 [m][N] (per_spot = 1; the explicit form always) or [N] for every spot (0), NULL = every hidden seat uniform
    const uint16_t *weights;
    uint32_t R;
    const uint16_t *range_of;
    int per_spot;
};

// Queues the whole call on `stream`: the R prefix sums, descriptors + zeroed outputs (one lane per spot), then the persistent sampling kernel.
// The task split is the sampled family's (eqs_lpt).  `tables` non-NULL selects the table form, whose `observer` is a seat or PK_OBSERVER_ACTIVE.
hipError_t eqw_launch(hipStream_t stream, const uint32_t *tab, const EqSpots *spots, const EqTables *tables, int observer, const EqsStream &rng,
                      const EqwRanges &ranges, int N, size_t m, const EqwOut &out, char *work);
// k_eqw_cdf alone, for another family that draws from the same rows (pk_ev_ranged.hip): cum u32 [R][1326]; R = 0 queues nothing
hipError_t eqw_launch_cdf(hipStream_t stream, const uint16_t *weights, uint32_t *cum, uint32_t R);
// the sampling kernel of one LDS size class (each class is an object file of its own: pokerl_amd/build.py)
template <int RC>
bool eqw_run_class(int n, hipStream_t stream, unsigned grid, const uint32_t *tab, const uint32_t *cum, const uint64_t *desc, const EqwOut &out,
                   const EqsStream &rng, uint32_t R, uint32_t ntasks, uint32_t nch, uint32_t per);

}  // namespace pk
