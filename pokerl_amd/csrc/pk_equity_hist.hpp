// pk_equity_hist.hpp -- strength histograms: for EVERY holding the hero can have on a public board, the distribution of its river strength
// against a weighted opponent range over the completions of the board (include/pokerl_hip.h "Strength histograms"):
// what the host entry points (pk_api.hip) and the kernels (pk_equity_hist.hip) share.  The spot, its check and its 3-word descriptor are
// those of range vs range (pk_equity_rvr.hpp: RvrSpots, RvrWeights, rvr_prep_launch, rvr_work_bytes).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pk_equity_rvr.hpp"

namespace pk {

constexpr int HIST_MAX_BINS = 32;                        // PK_EQ_HIST_MAX_BINS: 32 * 2 * 65 535 * C(45, 2) = 4 152 297 600 < 2^32
constexpr int HIST_COUNTS_BLOCK = 256;
static_assert(32ull * 2ull * 65535ull * 990ull < (1ull << 32), "the bin rule's largest product fits 32 bits");

struct HistOut {          // any may be NULL
    uint16_t *hist;          // [m][1326][nbins]
    uint16_t *void_;         // [m][1326]
    uint32_t *completions;   // [m]  C(P - 2, k): the completions ONE holding meets (not range vs range's boards = C(P - 4, k))
    uint8_t *status;         // [m]
};

// Queues the whole call on `stream`: k_rvr_prep (descriptors + status), the completions (one lane per spot) where they are wanted, then --
// where hist or void is wanted -- the persistent kernel.  1 <= nbins <= HIST_MAX_BINS is the caller's to check; `tables` non-NULL selects
// the table form.
hipError_t hist_launch(hipStream_t stream, const uint32_t *tab, const RvrSpots *spots, const EqTables *tables, const RvrWeights &weights, size_t m,
                       int nbins, const HistOut &out, uint64_t *desc);

}  // namespace pk
