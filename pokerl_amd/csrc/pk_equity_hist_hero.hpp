// pk_equity_hist_hero.hpp -- the hero form of the strength histograms: ONE seat's river-strength distribution against a weighted opponent range
// over the completions of the board, and optionally its bucket (include/pokerl_hip.h "Hero strength histogram"): what
// the host entry points (pk_api.hip) and the kernels (pk_equity_hist_hero.hip) share.  The spot, its check and its 4-word descriptor are those
// of range equity (pk_equity_range.hpp: EqrSpots, EqrWeights, eqr_prep_launch, eqr_work_bytes); the bucket stage is pk::cl_assign_launch
// (pk_hist_cluster.hpp) on the rows of the call.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pk_equity_range.hpp"
#include "pk_hist_cluster.hpp"

namespace pk {

constexpr int HH_MAX_BINS = 32;                          // PK_EQ_HIST_MAX_BINS: 32 * 2 * 65 535 * C(45, 2) < 2^32 (pk_equity_hist.hpp)
constexpr int HH_BLOCK = EQR_BLOCK, HH_WAVES = HH_BLOCK / 64;
constexpr int HH_GRID_MAX = EQR_GRID_MAX;                // persistent grid: three 512-thread workgroups per CU
constexpr int HH_COUNTS_BLOCK = 256;

struct HeroHistOut {      // any may be NULL
    uint16_t *hist;          // [m][nbins]
    uint16_t *void_;         // [m]
    uint32_t *completions;   // [m]  C(P, k): P counts the pool WITHOUT the hero's cards (range equity's boards is C(P - 2, k))
    uint8_t *status;         // [m]
};
struct HeroHistBucket {   // the optional bucket stage: K = 0 is none
    int K;
    const uint16_t *centroids;   // [K][nbins]
    uint16_t *label;             // [m]  either may be NULL
    uint32_t *dist;              // [m]
};

// The work space of a call, carved out of one buffer, every piece 256-byte aligned: the descriptors; with a bucket stage the rows (where
// the caller wants no hist), the labels (where the caller wants dist alone) and pk::cl_work_bytes.
size_t hh_work_bytes(size_t m, int nbins, const HeroHistOut &out, const HeroHistBucket &bk);

// Queues the whole call on `stream`: k_eqr_prep (descriptors + status), the completions (one lane per spot) where they are wanted, the
// persistent kernel where hist, void or a bucket is wanted, then the bucket stage.  Arguments are the caller's to check; `tables`
// non-NULL selects the table form (observer: a seat or PK_OBSERVER_ACTIVE).
hipError_t hh_launch(hipStream_t stream, const uint32_t *tab, const EqrSpots *spots, const EqTables *tables, int N, int observer,
                     const EqrWeights &weights, size_t m, int nbins, const HeroHistOut &out, const HeroHistBucket &bk, char *work);

}  // namespace pk
