// pk_ev_ranged.hpp -- ranged showdown EV in chips: the side pots of Game.end_hand (section 3.7's levels) over attempts drawn from weighted
// ranges (section 3.6's draw) (include/pokerl_hip.h "Ranged showdown EV"): what the host entry points (pk_api.hip)
// and the kernels (pk_ev_ranged.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pk_equity_ev.hpp"
#include "pk_equity_ranged.hpp"

namespace pk {

// A spot's descriptor: section 3.6's 8 + N words (eqw_desc_words), with one field more in word [3]:
//   [3] stream id | valid << 32 | groups << 40   (bit g of groups: group g of the spot's levels holds a level to COMPARE)
// A task is (spot, chunk of attempts, group of ev_group(N) levels); the tasks are ENUMERATED, m * nch * ev_groups_max(N) of them, and a
// task whose group has nothing to compare is skipped under a scalar branch (group 0 is never skipped: it counts the accepted attempts).
inline uint64_t evw_task_bound(int N, size_t m, uint32_t samples) { return eqs_task_bound(m, samples) * (uint64_t)ev_groups_max(N); }

// Work space of one call, laid out by evw_layout: section 3.6's (cumulative sums u32 [R][1326], descriptors), the level table, the bets as
// the kernels use them (the table form: bets + pending_bets), the amounts, and `share` / `accepted` when the caller did not ask for them.
struct EvwWork {
    uint32_t *cum;        // [R][1326]
    uint64_t *desc;       // [m][8 + N]
    uint32_t *levels;     // [m][N]: section 3.7's level records (EV_EXISTS | EV_LAST | EV_COMPARE, seat, remain mask)
    double *bets;         // [m][N]
    double *amount;       // [m][N]
    uint64_t *share;      // [m][N][N], NULL: the caller's array is used
    uint32_t *accepted;   // [m], NULL: the caller's array is used
};
size_t evw_layout(int N, size_t m, uint32_t R, bool own_share, bool own_accepted, char *base, EvwWork *w);

struct EvwOut {           // any but status may be NULL
    uint64_t *share;      // [m][N][N] level-major
    uint8_t *level_seat;  // [m][N]
    double *amount;       // [m][N]
    double *ev;           // [m][N]
    uint32_t *accepted;   // [m]
    uint8_t *status;      // [m]
};

// Queues the whole call on `stream`: the R prefix sums (k_eqw_cdf), k_evw_prep (checks, descriptor, levels, zeroed counters), the persistent
// sampling kernel k_evw<N, RC>, then k_evw_finish (the last stand's share cell and ev).  `tables` non-NULL selects the table form, whose
// `observer` is a seat or PK_OBSERVER_ACTIVE and whose bets are the handle's bets + pending_bets.
hipError_t evw_launch(hipStream_t stream, const uint32_t *tab, const EqSpots *spots, const double *bets, const EvTables *tables, int observer,
                      const EqsStream &rng, const EqwRanges &ranges, int N, size_t m, const EvwOut &out, const EvwWork &w);
// the sampling kernel of one LDS size class (each class is an object file of its own: pokerl_amd/build.py)
template <int RC>
bool evw_run_class(int n, hipStream_t stream, unsigned grid, const uint32_t *tab, const EvwWork &w, const EqsStream &rng, uint32_t R, uint32_t ntasks,
                   uint32_t nch, uint32_t per);

}  // namespace pk
