// pk_equity_rvr.hpp -- range against range: the exact win / tie / total weights of EVERY holding the hero can have on a public board against a
// weighted opponent range (include/pokerl_hip.h "Range vs range"): what the host entry points (pk_api.hip) and the
// kernels (pk_equity_rvr.hip) share.  The table kernels do not include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pk_equity.hpp"

namespace pk {

constexpr int RVR_HOLDINGS = PK_EQ_HOLDINGS;            // C(52, 2) unordered pairs: h = b (b - 1) / 2 + a, canonical indices a < b
constexpr int RVR_BLOCK = 512, RVR_WAVES = RVR_BLOCK / 64;
constexpr int RVR_PER_LANE = 3;                          // holdings a lane owns: h = tid, tid + 512, tid + 1024 (3 * 512 >= 1326)
constexpr int RVR_GRID_MAX = 512;                        // persistent grid: two 512-thread workgroups per CU (2 x ~62 KB of LDS)
constexpr int RVR_POOL_HOLDINGS = 1176;                  // C(49, 2): holdings of the largest pool (a full-pool flop), indexed by POOL SLOTS
constexpr int RVR_SLOTS = 2048;                          // sort slots: the next power of two
constexpr int RVR_PREFIX = RVR_BLOCK * RVR_PER_LANE;     // prefix sums: three sorted positions per lane, 1536 > 1081 = C(47, 2) ranked holdings
constexpr int RVR_DESC_WORDS = 3;
static_assert(RVR_BLOCK * RVR_PER_LANE >= RVR_HOLDINGS && RVR_BLOCK * RVR_PER_LANE >= RVR_POOL_HOLDINGS, "a lane owns at most RVR_PER_LANE holdings");
// A spot's descriptor: 3 64-bit words.
//   [0] known board cards: a suit-lane bit set OR(4 << Card.value), what eval7_tab_front_bits takes
//   [1] the pool: bit c set = the card of canonical index c (rank0 * 4 + suit) is not dead
//   [2] boards | k << 48 | P << 56   (k = 5 - nb cards to come, P = cards in the pool; boards = C(P - 4, k), 0 for a refused spot)
inline size_t rvr_work_bytes(size_t m) { return m * RVR_DESC_WORDS * sizeof(uint64_t); }

struct RvrSpots {         // the explicit form
    const uint8_t *board, *nboard;
    const uint64_t *dead;    // NULL: none
};
struct RvrOut {           // any may be NULL
    uint64_t *win, *tie, *tot;
    uint32_t *boards;
    uint8_t *status;
};
struct RvrWeights {
    const uint16_t *w;       // NULL: every weight is 1
    int per_spot;            // 0: one vector [1326] for the call, 1: [m][1326]
};

// What the two kernels of this spot (k_rvr, and k_hist of pk_equity_hist.hip) both name:
constexpr uint32_t RVR_NONE = 63;             // pool slot that holds no card: a completion card that does not exist (k < 2)
constexpr uint32_t RVR_SENT = 0xFFFFFFFFu;    // the key of a holding that is out of play on this completion: above every real key (24 bits)
static_assert(RVR_NONE == COMB_FROZEN, "pk::fill_pool empties that slot");

// Queues the whole call on `stream`: descriptors + boards / status (one lane per spot), then -- where win, tie or tot is wanted -- the
// persistent kernel.  tab: the evaluator table (eval7_table); `tables` non-NULL selects the table form.
hipError_t rvr_launch(hipStream_t stream, const uint32_t *tab, const RvrSpots *spots, const EqTables *tables, const RvrWeights &weights, size_t m,
                      const RvrOut &out, uint64_t *desc);
// The preparation kernel alone (m > 0): descriptors + boards / status (the win / tie / tot of `out` are not looked at).  The strength
// histograms (pk_equity_hist.hip) check their spots with it too: the same spot gets the same status from both families.
hipError_t rvr_prep_launch(hipStream_t stream, const RvrSpots *spots, const EqTables *tables, size_t m, const RvrOut &out, uint64_t *desc);

}  // namespace pk
